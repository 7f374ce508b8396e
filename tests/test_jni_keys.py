"""integration/jni/bmq_jni.c exports one Java_..._retain_store_gpu_NativeKeys_<name> symbol per native method of NativeKeys.java (the key
composer on the device: keys by id, the store, and match(limit, now) with keys), with the declarations the Java source carries.
(No JDK in this image: jni_min.h stands in for jni.h; the Java sources are not compiled.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JAVA = os.path.join(ROOT, "integration", "java", "org", "apache", "bifromq")


def test_key_natives_are_exported_and_declared(tmp_path):
    so = str(tmp_path / "libbmq_jni.so")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "integration", "jni"), "-o", so, os.path.join(ROOT, "integration", "jni", "bmq_jni.c"), "-L",
                    os.path.join(ROOT, "bifromq_amd"), "-lbmq"], check=True, capture_output=True, timeout=120)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"Java_org_apache_bifromq_retain_store_gpu_NativeKeys_(\w+)", syms))
    declared = set(re.findall(r"static native \w+ (\w+)\(", open(os.path.join(JAVA, "retain", "store", "gpu", "NativeKeys.java")).read()))
    assert declared == exported == {"retainKeysById", "retainKeysPrepare", "retainMatchKeys"}
    src = open(os.path.join(JAVA, "retain", "store", "gpu", "NativeKeys.java")).read()
    decl = re.search(r"static native long retainMatchKeys\(([^;]*)\);", src).group(1)
    assert len(decl.split(",")) == 16                                       # retainMatchLimited's 13 + outKeyOff, outKeys, needed2
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout
    assert {"bmq_retain_keys_by_id", "bmq_retain_keys_prepare", "bmq_retain_keys_match"} <= set(re.findall(r"U (bmq_\w+)", undefined))
