"""integration/jni/bmq_jni.c exports one Java_..._routes_gpu_NativeRoutes_<name> symbol per native method of NativeRoutes.java (bmq_routes_find:
route keys -> route ids on the device), with the declaration the Java source carries.
(No JDK in this image: jni_min.h stands in for jni.h; the Java sources are not compiled.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JAVA = os.path.join(ROOT, "integration", "java", "org", "apache", "bifromq")


def test_route_natives_are_exported_and_declared(tmp_path):
    so = str(tmp_path / "libbmq_jni.so")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "integration", "jni"), "-o", so, os.path.join(ROOT, "integration", "jni", "bmq_jni.c"), "-L",
                    os.path.join(ROOT, "bifromq_amd"), "-lbmq"], check=True, capture_output=True, timeout=120)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"Java_org_apache_bifromq_routes_gpu_NativeRoutes_(\w+)", syms))
    src = open(os.path.join(JAVA, "routes", "gpu", "NativeRoutes.java")).read()
    declared = set(re.findall(r"static native \w+ (\w+)\(", src))
    assert declared == exported == {"routesFind"}
    decl = re.search(r"static native void routesFind\(([^;]*)\);", src).group(1)
    assert [a.split()[0] for a in decl.split(",")] == ["long", "ByteBuffer", "IntBuffer", "int", "IntBuffer"]  # engine, keys, keyOff, n, outIds
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout
    assert "bmq_routes_find" in set(re.findall(r"U (bmq_\w+)", undefined))
