"""integration/jni/bmq_jni.c exports one Java_..._retain_store_gpu_NativeStore_<name> symbol per native method
integration/java/org/apache/bifromq/retain/store/gpu/NativeStore.java declares (the per-tenant statistics and the retain GC by id), and the
adapters beside it call nothing else.  (No JDK in this image: jni_min.h stands in for jni.h; the Java sources are not compiled.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JAVA = os.path.join(ROOT, "integration", "java", "org", "apache", "bifromq", "retain", "store", "gpu")


def test_native_store_symbols_match_the_java_declarations(tmp_path):
    so = str(tmp_path / "libbmq_jni.so")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "integration", "jni"), "-o", so, os.path.join(ROOT, "integration", "jni", "bmq_jni.c"), "-L",
                    os.path.join(ROOT, "bifromq_amd"), "-lbmq"], check=True, capture_output=True, timeout=120)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"Java_org_apache_bifromq_retain_store_gpu_NativeStore_(\w+)", syms))
    declared = set(re.findall(r"static native \w+ (\w+)\(", open(os.path.join(JAVA, "NativeStore.java")).read()))
    assert declared == exported == {"retainExpired", "retainGeneration", "retainMessageKeys", "retainRemoveIds", "retainTenantCounts", "routesTenantStats"}
    used = set()
    for name in ("GpuRetainGc.java", "GpuTenantsStats.java"):
        used |= set(re.findall(r"NativeStore\.(\w+)\(", open(os.path.join(JAVA, name)).read()))
    assert used == declared
