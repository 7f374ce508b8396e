"""integration/jni/bmq_jni.c exports one Java_..._retain_store_gpu_NativeRetainPlan_<name> symbol per native method of NativeRetainPlan.java (the
two halves of batchRetain around the KV commit), with the declarations the Java source carries, and GpuBatchRetain.java calls them with
those argument counts.  (No JDK in this image: jni_min.h stands in for jni.h; the Java sources are not compiled.)"""
import os
import re
import subprocess

from bifromq_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JAVA = os.path.join(ROOT, "integration", "java", "org", "apache", "bifromq", "retain", "store", "gpu")


def _args(text):
    return len([a for a in text.split(",") if a.strip()])


def test_plan_natives_are_exported_and_declared(tmp_path):
    so = str(tmp_path / "libbmq_jni.so")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "integration", "jni"), "-o", so, os.path.join(ROOT, "integration", "jni", "bmq_jni.c"), "-L",
                    os.path.join(ROOT, "bifromq_amd"), "-lbmq"], check=True, capture_output=True, timeout=120)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"Java_org_apache_bifromq_retain_store_gpu_NativeRetainPlan_(\w+)", syms))
    src = open(os.path.join(JAVA, "NativeRetainPlan.java")).read()
    declared = set(re.findall(r"static native \w+ (\w+)\(", src))
    assert declared == exported == {"retainPlan", "retainPlanCommit"}
    # Java arguments = the C ABI's minus keys_cap (the buffer's capacity) for the plan, one for one for the commit
    header = open(os.path.join(ROOT, "include", "bmq.h")).read()
    c_plan = _args(re.sub(r"/\*.*?\*/", "", re.search(r"\bint bmq_retain_plan\(([^;]*)\);", header).group(1), flags=re.S))
    c_commit = _args(re.sub(r"/\*.*?\*/", "", re.search(r"\bint bmq_retain_plan_commit\(([^;]*)\);", header).group(1), flags=re.S))
    j_plan = _args(re.search(r"static native long retainPlan\(([^;]*)\);", src).group(1))
    j_commit = _args(re.search(r"static native void retainPlanCommit\(([^;]*)\);", src).group(1))
    assert (c_plan, j_plan, c_commit, j_commit) == (18, 17, 14, 14)
    adapter = open(os.path.join(JAVA, "GpuBatchRetain.java")).read()
    calls = re.findall(r"NativeRetainPlan\.retainPlan\(([^;]*)\);", adapter)
    assert len(calls) == 2 and all(_args(c) == j_plan for c in calls)
    assert _args(re.search(r"NativeRetainPlan\.retainPlanCommit\(([^;]*)\);", adapter).group(1)) == j_commit
    for name, value in re.findall(r"\b(NONE|ADD|UPDATE|REMOVE|SUPERSEDED) = (\d)", src):
        assert re.search(r"BMQ_PLAN_%s = %s\b" % (name, value), header), name
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout
    assert {"bmq_retain_plan", "bmq_retain_plan_commit"} <= set(re.findall(r"U (bmq_\w+)", undefined)) <= set(_lib.ABI_SYMBOLS)
