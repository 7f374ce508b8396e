"""integration/jni/bmq_jni.c exports one Java_..._retain_store_gpu_NativeRange_<name> symbol per native method
integration/java/org/apache/bifromq/retain/store/gpu/NativeRange.java declares (the retain store's split and merge by KV boundary), and the
reset(Boundary) adapter beside it, GpuRetainRange.java, calls nothing else.  (No JDK in this image: jni_min.h stands in for jni.h; the Java
sources are not compiled.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JAVA = os.path.join(ROOT, "integration", "java", "org", "apache", "bifromq")


def test_native_range_symbols_match_the_java_declarations(tmp_path):
    so = str(tmp_path / "libbmq_jni.so")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "integration", "jni"), "-o", so, os.path.join(ROOT, "integration", "jni", "bmq_jni.c"), "-L",
                    os.path.join(ROOT, "bifromq_amd"), "-lbmq"], check=True, capture_output=True, timeout=120)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"Java_org_apache_bifromq_retain_store_gpu_NativeRange_(\w+)", syms))
    declared = set(re.findall(r"static native \w+ (\w+)\(", open(os.path.join(JAVA, "retain", "store", "gpu", "NativeRange.java")).read()))
    assert declared == exported == {"retainCountIn", "retainIdsIn", "retainCompactBeginIn", "retainReset", "retainImport"}
    adapter = open(os.path.join(JAVA, "retain", "store", "gpu", "GpuRetainRange.java")).read()
    used = set(re.findall(r"NativeRange\.(\w+)\(", adapter))
    assert used == declared - {"retainCompactBeginIn"}      # (retainReset is begin_in + build + swap in one call)
    assert not re.findall(r"Native(?:Matcher|Store|Keys)\.\w+\(", adapter)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ("bmq_retain_count_in", "bmq_retain_ids_in", "bmq_retain_compact_begin_in", "bmq_retain_compact_build", "bmq_retain_compact_swap", "bmq_retain_import"):
        assert re.search(r"\b%s\b" % name, undefined), name
