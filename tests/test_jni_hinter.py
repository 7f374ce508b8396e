"""integration/jni/bmq_jni.c exports the Java_..._routes_gpu_NativeHinter_routesPrefixCensus symbol NativeHinter.java declares (bmq_routes_prefix_census:
the live routes under each key prefix of a mutation batch, in one pass on the device), and the adapter GpuFanoutSplitHinter.java calls it and the
key-ordered window.  (No JDK in this image: jni_min.h stands in for jni.h; the Java sources are not compiled.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JAVA = os.path.join(ROOT, "integration", "java", "org", "apache", "bifromq", "routes", "gpu")


def test_the_hinter_native_is_exported_declared_and_called(tmp_path):
    so = str(tmp_path / "libbmq_jni.so")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "integration", "jni"), "-o", so, os.path.join(ROOT, "integration", "jni", "bmq_jni.c"), "-L",
                    os.path.join(ROOT, "bifromq_amd"), "-lbmq"], check=True, capture_output=True, timeout=120)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"Java_org_apache_bifromq_routes_gpu_NativeHinter_(\w+)", syms))
    src = open(os.path.join(JAVA, "NativeHinter.java")).read()
    declared = set(re.findall(r"static native \w+ (\w+)\(", src))
    assert declared == exported == {"routesPrefixCensus"}
    args = [a.split()[0] for a in re.search(r"static native void routesPrefixCensus\(([^;]*)\);", src).group(1).split(",")]
    assert args == ["long", "ByteBuffer", "IntBuffer", "int", "LongBuffer"]  # engine, prefixes, prefixOff, n, outStats
    undefined = set(re.findall(r"U (bmq_\w+)", subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout))
    assert "bmq_routes_prefix_census" in undefined  # the shim calls the library, it does not carry a copy
    adapter = open(os.path.join(JAVA, "GpuFanoutSplitHinter.java")).read()
    assert "implements IKVRangeSplitHinter" in adapter and "NativeHinter.routesPrefixCensus(" in adapter and "NativeGc.routesWindow(" in adapter
    assert "BoundaryUtil.isSplittable" in adapter and "BoundaryUtil.inRange" in adapter
    assert re.search(r"PREFIX_MAX = 65536;", src)


def test_header_library_and_bindings_agree_on_the_new_symbols():
    from bifromq_amd import _lib
    header = open(os.path.join(ROOT, "include", "bmq.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "bifromq_amd", "libbmq.so")], capture_output=True, text=True, check=True).stdout
    for name in ("bmq_routes_prefix_census", "bmq_routes_prefix_census_info_get"):
        assert re.search(r"\bint %s\(" % name, header) and re.search(r" T %s\b" % name, syms) and name in _lib.ABI_SYMBOLS, name
    assert re.search(r"#define BMQ_PREFIX_MAX 65536u", header)
    import bifromq_amd as B
    assert B.BMQ_PREFIX_MAX == 65536 == B.Engine(device=-1).prefix_census_info().prefix_max
