"""The support and size queries of the depthwise-conv C ABI pinned (no GPU needed: they are host code, and without a device the CU count they
use falls back to the MI355X's 256).  tests/golden/dispatch_queries.npz holds what every query of tools/print_dispatch.py's QUERY_GRID answered,
and what the 12 stage shapes answered with each A/B switch of QUERY_SWITCHES off, recorded before the selection functions of capi.hip were
written (python tools/print_dispatch.py --queries ...).  A kernel family that goes in at the wrong rung of one ladder changes an entry here."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("_print_dispatch", os.path.join(HERE, "..", "tools", "print_dispatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cu = ctypes.c_int(0)
    if mod.load_lib().slak_device_info(ctypes.byref(cu), None, None, 0) == 0 and cu.value != 256:
        pytest.skip("recorded for 256 CUs; this device has %d" % cu.value)
    return mod


@pytest.fixture(scope="module")
def want():
    return dict(np.load(os.path.join(HERE, "golden", "dispatch_queries.npz"), allow_pickle=False))


def _same(got, want, points, what):
    got = np.asarray(got, dtype=np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d entries differ, first (dtype, N, C, H, W, K) = %s column %d: got %d, recorded %d" % (
        what, len(bad), points[bad[0][0]], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


def test_queries_over_the_grid_answer_what_was_recorded(tool, want):
    assert want["grid"].shape == (len(tool.QUERY_GRID), tool.QUERY_COLUMNS)
    _same(tool.queries(tool.load_lib(), tool.QUERY_GRID), want["grid"], tool.QUERY_GRID, "grid")


def test_queries_with_each_switch_off_answer_what_was_recorded(tool, want):
    assert sorted(want) == sorted(["grid"] + tool.QUERY_SWITCHES)
    for name in tool.QUERY_SWITCHES:            # a fresh process per switch: switches are read once per process
        _same(tool.stage_queries_with_switch_off(name), want[name], tool.STAGE_POINTS, name + "=0")
