"""integration/jni/bmq_jni.c exports one Java_..._routes_gpu_NativeGc_<name> symbol per native method of NativeGc.java (bmq_routes_window,
bmq_routes_gc_sweep: reads of the route keys in key order on the device), with the declarations the Java source carries, and the adapter
GpuRouteGc.java calls them.  (No JDK in this image: jni_min.h stands in for jni.h; the Java sources are not compiled.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JAVA = os.path.join(ROOT, "integration", "java", "org", "apache", "bifromq", "routes", "gpu")


def test_gc_natives_are_exported_and_declared(tmp_path):
    so = str(tmp_path / "libbmq_jni.so")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "integration", "jni"), "-o", so, os.path.join(ROOT, "integration", "jni", "bmq_jni.c"), "-L",
                    os.path.join(ROOT, "bifromq_amd"), "-lbmq"], check=True, capture_output=True, timeout=120)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"Java_org_apache_bifromq_routes_gpu_NativeGc_(\w+)", syms))
    src = open(os.path.join(JAVA, "NativeGc.java")).read()
    declared = set(re.findall(r"static native \w+ (\w+)\(", src))
    assert declared == exported == {"routesWindow", "routesGcSweep", "routeKey"}
    args = lambda name: [a.split()[0] for a in re.search(r"static native int %s\(([^;]*)\);" % name, src).group(1).split(",")]  # noqa: E731
    assert args("routesWindow") == ["long", "ByteBuffer", "int", "boolean", "int", "IntBuffer", "IntBuffer"]  # engine, lo, loLen, exclusive, maxRoutes, outIds, outMore
    assert args("routesGcSweep") == ["long", "ByteBuffer", "int", "int", "int", "IntBuffer", "int", "LongBuffer"]  # engine, startKey, startLen, stepHint, scanQuota, outIds, cap, reply
    undefined = set(re.findall(r"U (bmq_\w+)", subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout))
    assert {"bmq_routes_window", "bmq_routes_gc_sweep", "bmq_route_key"} <= undefined
    adapter = open(os.path.join(JAVA, "GpuRouteGc.java")).read()
    assert args("routeKey") == ["long", "int", "ByteBuffer"]  # engine, routeId, out
    assert "NativeGc.routesGcSweep(" in adapter and "NativeGc.routeKey(" in adapter and "BoundaryUtil.compareEndKeys" in adapter


def test_header_library_and_bindings_agree_on_the_new_symbols():
    from bifromq_amd import _lib
    header = open(os.path.join(ROOT, "include", "bmq.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "bifromq_amd", "libbmq.so")], capture_output=True, text=True, check=True).stdout
    for name in ("bmq_routes_window", "bmq_routes_gc_sweep", "bmq_routes_window_info_get"):
        assert re.search(r"\bint %s\(" % name, header) and re.search(r" T %s\b" % name, syms) and name in _lib.ABI_SYMBOLS, name
    assert re.search(r"#define BMQ_WINDOW_MAX 65536u", header)
    import bifromq_amd as B
    assert B.BMQ_WINDOW_MAX == 65536 == B.Engine(device=-1).window_info().window_max
