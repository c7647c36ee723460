"""slak_tri_plan (include/slak_hip.h) pinned: the one place where the launch ladder of a block's three branch convs is decided (no GPU needed: the
query is host code, and without a device the CU count it uses falls back to the MI355X's 256).  tests/golden/tri_plan.json holds what the ladder,
restated from the primitive slak_dwconv2d_tri_* / _pair_* queries by tests/golden/make_tri_plan_golden.py on a library from before the query
existed, answers on dtype x shape x allow; the query must answer the same on every point, and the recording must contain every rung of every field."""
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
    """slak_tri_plan over the golden script's GRID as rows of its FIELDS (the binding loaded by path: no torch in the child processes)."""
    gold, _lib = _load("golden/make_tri_plan_golden.py", "_tri_plan_golden"), _load("../slak_amd/_lib.py", "_slak_lib_only")
    L, out = _lib.lib(), []
    for point in gold.GRID:
        p = _lib.TriPlan()
        assert L.slak_tri_plan(*point, ctypes.byref(p)) == 0, point
        out.append([int(getattr(p, f)) for f in gold.FIELDS])
    return out


@pytest.fixture(scope="module")
def gold():
    mod = _load("golden/make_tri_plan_golden.py", "_tri_plan_golden")
    cu = ctypes.c_int(0)
    if _load("../slak_amd/_lib.py", "_slak_lib_only").lib().slak_device_info(ctypes.byref(cu), None, None, 0) == 0 and cu.value != 256:
        pytest.skip("recorded for 256 CUs; this device has %d" % cu.value)
    return mod


@pytest.fixture(scope="module")
def want(gold):
    doc = json.load(open(os.path.join(HERE, "golden", "tri_plan.json")))
    assert doc["fields"] == gold.FIELDS and (doc["dtype"], [tuple(s) for s in doc["shape"]], doc["allow"]) == (gold.DTYPES, gold.SHAPES, gold.ALLOWS)
    assert sorted(doc["rows"]) == sorted(["default"] + ["%s=%s" % s for s in gold.SWITCHES])
    assert all(len(r) == len(gold.GRID) for r in doc["rows"].values())
    return doc["rows"]


def _same(got, want, gold, what):
    bad = [(p, g, w) for p, g, w in zip(gold.GRID, got, want) if g != w]
    assert len(got) == len(want) and not bad, "%s: %d of %d points differ, first (dtype, N, C, H, W, K, allow) = %s: slak_tri_plan %s, recorded %s (%s)" % (
        what, len(bad), len(want), bad[0][0], bad[0][1], bad[0][2], gold.FIELDS)


def test_plan_is_the_recorded_ladder_on_every_grid_point(gold, want):
    _same(plan_rows(), want["default"], gold, "default switches")


def test_plan_is_the_recorded_ladder_under_a_library_switch(gold, want):
    for name, value in gold.SWITCHES:           # a fresh process per switch: the library reads it once
        _same(gold.in_child(os.path.abspath(__file__), name, value), want["%s=%s" % (name, value)], gold, "%s=%s" % (name, value))


def test_plan_checks_its_arguments():
    _lib = _load("../slak_amd/_lib.py", "_slak_lib_only")
    L, p = _lib.lib(), _lib.TriPlan()
    assert L.slak_tri_plan(_lib.SLAK_BF16, 2, 2, 7, 7, 13, _lib.TRI_ALLOW_ALL, None) == 1            # SLAK_ERR_INVALID_ARG
    for bad in ((0, 2, 7, 7, 13), (2, 0, 7, 7, 13), (2, 2, 0, 7, 13), (2, 2, 7, -1, 13), (2, 2, 7, 7, 0)):
        assert L.slak_tri_plan(_lib.SLAK_BF16, *bad, _lib.TRI_ALLOW_ALL, ctypes.byref(p)) == 1, bad


def test_recording_holds_every_rung_of_every_field(gold, want):
    """A grid that misses a rung pins nothing about it."""
    g = gold
    seen = lambda rows: {f: {r[i] for r in rows} for i, f in enumerate(g.FIELDS)}
    every = seen([r for rows in want.values() for r in rows])
    assert every["fwd"] == {g.FWD_TRI_STATS, g.FWD_TRI, g.FWD_BRANCH_STATS, g.FWD_BRANCH}
    assert every["dgrad"] == {g.DGRAD_ONE, g.DGRAD_TRI, g.DGRAD_BRANCH_ACC, g.DGRAD_BRANCH_ADD}
    assert every["wgrad"] == {g.WGRAD_ONE, g.WGRAD_TRI, g.WGRAD_PAIR, g.WGRAD_BRANCH}
    assert 0 in every["stats_rows"] and max(every["stats_rows"]) > 1 and 0 in every["ws_wgrad"] and max(every["ws_wgrad"]) > 0
    for r in (r for rows in want.values() for r in rows):                         # the fields hang together as the header says
        fwd, stats_rows, dgrad, wgrad, ws = r
        assert (stats_rows > 0) == (fwd == g.FWD_TRI_STATS) and (dgrad == g.DGRAD_ONE) == (wgrad == g.WGRAD_ONE), r
        assert (ws > 0) == (wgrad != g.WGRAD_BRANCH), r
    # at the default switches every rung but PAIR is there (the three-branch weight gradient shadows it); each library switch moves what it names
    default = seen(want["default"])
    assert default["fwd"] == every["fwd"] and default["dgrad"] == every["dgrad"] and default["wgrad"] == every["wgrad"] - {g.WGRAD_PAIR}
    assert g.WGRAD_PAIR in seen(want["SLAK_TRI_ROWS=0"])["wgrad"] and g.WGRAD_PAIR in seen(want["SLAK_TRI_WAVE=0"])["wgrad"]
    assert g.DGRAD_ONE not in seen(want["SLAK_SMALL_TRI_BWD=0"])["dgrad"] and g.DGRAD_ONE in default["dgrad"]
    assert seen(want["SLAK_WGRAD_REDUCE=1"])["wgrad"] == {g.WGRAD_BRANCH}
    assert all(rows != want["default"] for name, rows in want.items() if name != "default")


if __name__ == "__main__":                      # the child of test_plan_is_the_recorded_ladder_under_a_library_switch
    assert "--rows" in sys.argv
    print(json.dumps(plan_rows()))
