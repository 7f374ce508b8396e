"""The model of the dist worker's GC sweep (tests/gc_sweep_ref.py) against the cases of the reference's own test
(tests/golden/gc_sweep_cases.json: DistWorkerCoProcGCTest.java:120-232 as data), and the brute-force window against hand-made answers.
tests/test_gc_sweep.py and tests/test_gc_sweep_gpu.py compare the engine with this model."""
import json
import os

import pytest

import bifromq_amd as B
from tests import gc_sweep_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gc_sweep_cases.json")


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def case_keys(case):
    return sorted(B.route_key(k["tenant"], k["filter"], k["flag"], k["receiver"]) for k in case["keys"])


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"].split(",")[0].replace(" ", "_")[:48])
def test_the_model_gives_what_the_reference_test_asserts(case):
    ks = case_keys(case)
    assert len(set(ks)) == len(case["keys"])
    start = None if case["start"] is None else ks[case["start"]]
    inspected, wrapped, nxt = R.sweep(ks, start, case["step"], case["quota"])
    a, d = case["reference_asserts"], case["derived"]
    if "inspected" in a:
        assert len(inspected) == a["inspected"]
    if "inspected_at_least" in a:
        assert len(inspected) >= a["inspected_at_least"]
    if "wrapped" in a:
        assert wrapped == a["wrapped"]
    if "has_next" in a:
        assert (nxt is not None) == a["has_next"]
    assert inspected == [ks[p] for p in d["inspected_positions"]]
    assert wrapped == d["wrapped"]
    assert nxt == (None if d["next_position"] is None else ks[d["next_position"]])


def test_the_model_in_words():
    ks = [b"a", b"b", b"c", b"d", b"e"]
    assert R.sweep(ks, b"z") == ([], True, None)  # past the end: nothing, although keys lie in front of the cursor
    assert R.sweep(ks, b"bb", 1, 2) == ([b"c", b"d"], False, b"e")
    assert R.sweep(ks, b"d", 1, 0) == ([b"d", b"e", b"a", b"b", b"c"], True, b"d")
    assert R.sweep(ks, b"d", 2, 3) == ([b"d", b"a", b"c"], True, b"d")  # the quota moves the cursor ONE on: onto the start key here
    assert R.sweep(ks, b"a", 1, 5) == ([b"a", b"b", b"c", b"d", b"e"], False, None)
    assert R.sweep(ks, b"b", 3, 0) == ([b"b", b"e", b"a", b"d"], True, None)  # jumps over b after the wrap, then the tail again
    assert R.sweep(ks, b"0", 1, 1, boundary=(b"c", None)) == ([b"c"], False, b"d")  # below the boundary's start: clamped
    assert R.sweep(ks, b"e", 1, 1, boundary=(b"b", b"e")) == ([b"b"], False, b"c")  # at the boundary's end: clamped to the start
    assert R.sweep(ks, b"e", 1, 1, boundary=(None, b"e")) == ([b"a"], False, b"b")  # ... which may be absent: from the first key


def test_the_brute_force_window():
    ks = [b"b", b"a\x80", b"a", b"ab", b"\xff", b""]
    assert R.window(ks) == ([b"", b"a", b"ab", b"a\x80", b"b", b"\xff"], False)  # unsigned bytes, a proper prefix first
    assert R.window(ks, b"a", 2) == ([b"a", b"ab"], True)
    assert R.window(ks, b"a", 2, exclusive=True) == ([b"ab", b"a\x80"], True)
    assert R.window(ks, b"a\x00", 9) == ([b"ab", b"a\x80", b"b", b"\xff"], False)
    assert R.window(ks, b"\xff", 1) == ([b"\xff"], False)
    assert R.window(ks, b"\xff", 1, exclusive=True) == ([], False)
    assert R.window(ks, b"", 0) == ([], True)
