"""slak_mlp_plan (include/slak_hip.h) pinned: the one place where the kernel ladder of a block's pointwise MLP is decided (no GPU needed: the
query is host code, and without a device the CU count it uses falls back to the MI355X's 256).  tests/golden/mlp_plan.json holds what the ladder,
restated from the primitive *_supported / *_workspace_bytes queries by tests/golden/make_mlp_plan_golden.py on a library from before the query
existed, answers on M x Cp x allow; the query must answer the same on every point, and the recording must contain every rung of every step."""
import ctypes
import importlib.util
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plan_rows():
    """slak_mlp_plan over the golden script's GRID as rows of its FIELDS (the binding loaded by path: no torch in the child processes)."""
    gold, _lib = _load("golden/make_mlp_plan_golden.py", "_mlp_plan_golden"), _load("../slak_amd/_lib.py", "_slak_lib_only")
    L, out = _lib.lib(), []
    for M, C4, Cp, allow in gold.GRID:
        p = _lib.MlpPlan()
        assert L.slak_mlp_plan(M, C4, Cp, allow, ctypes.byref(p)) == 0, (M, C4, Cp, allow)
        out.append([int(getattr(p, f)) for f in gold.FIELDS])
    return out


@pytest.fixture(scope="module")
def gold():
    mod = _load("golden/make_mlp_plan_golden.py", "_mlp_plan_golden")
    cu = ctypes.c_int(0)
    if _load("../slak_amd/_lib.py", "_slak_lib_only").lib().slak_device_info(ctypes.byref(cu), None, None, 0) == 0 and cu.value != 256:
        pytest.skip("recorded for 256 CUs; this device has %d" % cu.value)
    return mod


@pytest.fixture(scope="module")
def want(gold):
    doc = json.load(open(os.path.join(HERE, "golden", "mlp_plan.json")))
    assert doc["fields"] == gold.FIELDS and (doc["M"], doc["Cp"], doc["allow"]) == (gold.MS, gold.CPS, gold.ALLOWS)
    assert sorted(doc["rows"]) == sorted(["default"] + [s + "=0" for s in gold.SWITCHES])
    assert all(len(r) == len(gold.GRID) for r in doc["rows"].values())
    return doc["rows"]


def _same(got, want, gold, what):
    bad = [(p, g, w) for p, g, w in zip(gold.GRID, got, want) if g != w]
    assert len(got) == len(want) and not bad, "%s: %d of %d points differ, first (M, C4, Cp, allow) = %s: slak_mlp_plan %s, recorded %s (%s)" % (
        what, len(bad), len(want), bad[0][0], bad[0][1], bad[0][2], gold.FIELDS)


def test_plan_is_the_recorded_ladder_on_every_grid_point(gold, want):
    _same(plan_rows(), want["default"], gold, "default switches")


def test_plan_is_the_recorded_ladder_with_a_library_switch_off(gold, want):
    for name in gold.SWITCHES:                  # a fresh process per switch: the library reads it once
        _same(gold.in_child(os.path.abspath(__file__), name), want[name + "=0"], gold, name + "=0")


def test_recording_holds_every_rung_of_every_step(gold, want):
    """A grid that misses a rung pins nothing about it."""
    seen = {f: set() for f in gold.FIELDS}
    for rows in want.values():
        for r in rows:
            for f, v in zip(gold.FIELDS, r):
                seen[f].add(v)
    g = gold
    assert seen["pw1"] == {g.FUSED, g.NT, g.GEMM, g.LIBRARY}
    assert seen["pw2"] == {g.NT, g.LIBRARY} and seen["dt"] == {g.NT, g.LIBRARY}
    assert seen["dy1"] == {g.FUSED_DT, g.FUSED, g.GEMM, g.NT, g.LIBRARY}
    assert seen["dw1"] == {g.KERNEL, g.LIBRARY} and seen["dw2"] == {g.KERNEL, g.LIBRARY}
    assert {1, 2, 4, 64} <= seen["splits"]                  # one plain GEMM, and the rule at M = 6272 k
    assert 0 in seen["ws_dw1"] and max(seen["ws_dw1"]) > 0 and min(seen["ws_dy1"]) > 0
    # the rungs a reader would expect at the default switches ARE there at the default switches (not only under a library switch)
    default = {f: {r[i] for r in want["default"]} for i, f in enumerate(gold.FIELDS)}
    assert default["pw1"] == {g.FUSED, g.GEMM, g.LIBRARY} and default["dy1"] == {g.FUSED_DT, g.GEMM, g.NT, g.LIBRARY}


if __name__ == "__main__":                      # the child of test_plan_is_the_recorded_ladder_with_a_library_switch_off
    assert "--rows" in sys.argv
    print(json.dumps(plan_rows()))
