// bmq_control.h -- what the controls of the stages behind a match (bmq_fanout.h, bmq_share.h, bmq_delivery.h, bmq_caps.h, bmq_gate.h) have
// in common over their Exec: the error string, the release of exec memory and, for those that own grow-only scratch, the buffer type with
// the ONE ensure -- the place where a buffer that grows is freed, behind a sync of the stream and through the before_free hook.
#pragma once
#include <functional>
#include <string>

namespace bmq {

template <class Exec> class ControlBase {
public:
    ControlBase(const ControlBase&) = delete;
    ControlBase& operator=(const ControlBase&) = delete;

    std::string error;

protected:
    explicit ControlBase(Exec& exec) : x(exec) {}
    Exec& x;

    template <class T> void rel(T*& p) {
        if (p) x.release(p);
        p = nullptr;
    }
    bool fail(const std::string& m) {
        error = m;
        return false;
    }
    bool xfail() { return fail(x.err.empty() ? "exec failure" : x.err); }
};

template <class Exec> class Control : public ControlBase<Exec> {
public:
    bool invalid = false;              // the last failure was the caller's input
    std::function<void()> before_free; // called before exec memory is released (a buffer that grows)

protected:
    using ControlBase<Exec>::x;
    explicit Control(Exec& exec) : ControlBase<Exec>(exec) {}

    bool bad(const std::string& m) {
        invalid = true;
        return this->fail(m);
    }
    // grow-only scratch in exec memory: pointer and capacity (in elements) together; released with the control that declares it
    template <class T> struct Scratch {
        explicit Scratch(Control& c) : x(c.x) {}
        ~Scratch() {
            if (p) x.release(p);
        }
        Scratch(const Scratch&) = delete;
        Scratch& operator=(const Scratch&) = delete;
        operator T*() const { return p; }
        Exec& x;
        T* p = nullptr;
        size_t cap = 0;
    };
    // contents dropped; a buffer in use by the stream is not freed under it, and the free goes through the hook
    template <class T> bool ensure(Scratch<T>& s, size_t need) {
        if (need <= s.cap && s.p) return true;
        if (!x.sync()) return this->xfail();
        if (s.p && before_free) before_free();
        this->rel(s.p);
        s.cap = 0;
        const size_t want = need + need / 4 + 64;
        s.p = (T*)x.alloc(want * sizeof(T) + 16);
        if (!s.p) return this->fail("out of memory");
        s.cap = want;
        return true;
    }
};

} // namespace bmq
