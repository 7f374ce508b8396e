// bmq_key_core.h -- the pieces of the retain store key schema that run on the host AND on the device: the UTF-8 -> UTF-16 walk behind
// Java's String.hashCode / LevelHash (bifromq-retain-store-schema/.../schema/LevelHash.java:30-50), the FNV-1a step, and the layout of
// retainMessageKey (KVSchemaUtil.java:44-73).  ONE definition: bmq_codec.cpp (host strings) and bmq_retain_core.h (the key kernels of
// bmq_exec_dev.h, HostExec for host-only engines and the fuzzers) both call these.
//
//   retainMessageKey(tenant, topic) = 0x00 | u16be(len tenant) | tenant | u16be(#levels) | one LevelHash byte per level | topic, '/' -> 0x00
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bmq_layout.h"

namespace bmq {

// The code point that starts at s[i] (i < n), i moved behind it.  A lead byte whose sequence does not fit into [i, n) and a byte that
// is no lead byte give U+FFFD and consume ONE byte; continuation bytes are taken as they are (their top bits are not checked).
BMQ_HD uint32_t utf8_next(const uint8_t* s, size_t n, size_t& i) {
    const uint32_t c = s[i];
    if (c < 0x80) {
        i += 1;
        return c;
    }
    if ((c & 0xE0) == 0xC0 && i + 1 < n) {
        const uint32_t cp = ((c & 0x1F) << 6) | (s[i + 1] & 0x3Fu);
        i += 2;
        return cp;
    }
    if ((c & 0xF0) == 0xE0 && i + 2 < n) {
        const uint32_t cp = ((c & 0x0F) << 12) | ((s[i + 1] & 0x3Fu) << 6) | (s[i + 2] & 0x3Fu);
        i += 3;
        return cp;
    }
    if ((c & 0xF8) == 0xF0 && i + 3 < n) {
        const uint32_t cp = ((c & 0x07) << 18) | ((s[i + 1] & 0x3Fu) << 12) | ((s[i + 2] & 0x3Fu) << 6) | (s[i + 3] & 0x3Fu);
        i += 4;
        return cp;
    }
    i += 1;
    return 0xFFFDu;
}

// f(unit) for every UTF-16 code unit of the UTF-8 string s[0, n): a code point from U+10000 on as its surrogate pair
template <class F> BMQ_HD void for_each_utf16_unit(const uint8_t* s, size_t n, F&& f) {
    size_t i = 0;
    while (i < n) {
        uint32_t cp = utf8_next(s, n, i);
        if (cp >= 0x10000) {
            cp -= 0x10000;
            f(0xD800u + (cp >> 10));
            f(0xDC00u + (cp & 0x3FF));
        } else f(cp);
    }
}

constexpr uint32_t FNV1A_INIT = 0x811C9DC5u;
BMQ_HD uint32_t fnv1a_step(uint32_t h, uint32_t unit) { return (h ^ unit) * 0x01000193u; }

// LevelHash of one level: FNV-1a 32 over its UTF-16 code units, lowest byte
BMQ_HD uint8_t level_hash_byte(const uint8_t* s, size_t n) {
    uint32_t h = FNV1A_INIT;
    size_t i = 0;
    while (i < n) { // (for_each_utf16_unit without the callable: this is the loop the key kernels run)
        uint32_t cp = utf8_next(s, n, i);
        if (cp >= 0x10000) {
            cp -= 0x10000;
            h = fnv1a_step(h, 0xD800u + (cp >> 10));
            h = fnv1a_step(h, 0xDC00u + (cp & 0x3FF));
        } else h = fnv1a_step(h, cp);
    }
    return (uint8_t)(h & 0xFF);
}

// length of retainMessageKey for a tenant id of tl bytes and a topic of pl bytes in `levels` levels
BMQ_HD uint32_t retain_key_len(uint32_t tl, uint32_t pl, uint32_t levels) { return 3u + tl + 2u + levels + pl; }

// 0x00 | u16be(tl) | tenant; returns the bytes written (3 + tl).  The lengths go in modulo 2^16, as the host encoder writes them.
BMQ_HD uint32_t retain_key_head(uint8_t* out, const uint8_t* tenant, uint32_t tl) {
    out[0] = 0;
    out[1] = (uint8_t)((tl >> 8) & 0xFF);
    out[2] = (uint8_t)(tl & 0xFF);
    for (uint32_t k = 0; k < tl; k++) out[3 + k] = tenant[k];
    return 3u + tl;
}

// The part behind the tenant for a topic that lies in ONE piece: u16be(levels) | a LevelHash byte per level | the topic, '/' -> 0x00.
// out has room for 2 + levels + pl bytes; `levels` = separators + 1 (TopicUtil.parse keeps empty levels).
BMQ_HD void retain_key_tail(uint8_t* out, const uint8_t* topic, uint32_t pl, uint32_t levels) {
    out[0] = (uint8_t)((levels >> 8) & 0xFF);
    out[1] = (uint8_t)(levels & 0xFF);
    uint8_t* hash = out + 2;
    uint8_t* body = out + 2 + levels;
    uint32_t b = 0, lv = 0;
    for (uint32_t i = 0; i <= pl; i++) {
        if (i < pl && topic[i] != '/') {
            body[i] = topic[i];
            continue;
        }
        if (lv < levels) hash[lv] = level_hash_byte(topic + b, i - b);
        lv++;
        if (i < pl) body[i] = 0; // TopicUtil.escape
        b = i + 1;
    }
}

} // namespace bmq
