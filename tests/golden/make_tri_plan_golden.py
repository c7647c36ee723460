"""Writes tests/golden/tri_plan.json: which entry point runs each step of a block's three branch convs, for every point of GRID.

    python tests/golden/make_tri_plan_golden.py [--lib PATH/libslak_hip.so] [--out PATH.json]

The independent restatement of the ladder that slak_tri_plan (include/slak_hip.h) answers: evaluated here from the primitive slak_dwconv2d_tri_* /
_pair_* queries ONLY -- this script never calls slak_tri_plan, so it runs unchanged on a library from before that query existed (the recording was
made on such a library and on the first one with the query: byte-identical files).  Host code only, no GPU needed; without a device the CU count the
queries use falls back to the MI355X's 256 (tests/test_tri_plan_cpu.py skips on a device with another count).

At the default switches the two-branch weight gradient (PAIR) appears on no shape: the three-branch launch shadows it wherever it applies.  The
library's own A/B switches SLAK_TRI_ROWS=0 and SLAK_TRI_WAVE=0 uncover it, SLAK_SMALL_TRI_BWD=0 takes the one-launch backward away and
SLAK_WGRAD_REDUCE=1 every fused weight gradient; each is recorded over the whole grid by a child process (the library reads a switch once per
process)."""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "..", "..", "slak_amd", "lib", "libslak_hip.so")
BF16, F16 = 2, 1                                                       # SLAK_BF16, SLAK_F16 of include/slak_hip.h
FWD_BRANCH, FWD_BRANCH_STATS, FWD_TRI, FWD_TRI_STATS = 0, 1, 2, 3      # SLAK_TRI_FWD_*
DGRAD_BRANCH_ADD, DGRAD_BRANCH_ACC, DGRAD_TRI, DGRAD_ONE = 0, 1, 2, 3  # SLAK_TRI_DGRAD_*
WGRAD_BRANCH, WGRAD_PAIR, WGRAD_TRI, WGRAD_ONE = 0, 1, 2, 3            # SLAK_TRI_WGRAD_*
FUSED, STATS, WGRAD, BACKWARD, DGRAD_ACC, ALL = 1, 2, 4, 8, 16, 31     # SLAK_TRI_ALLOW_*
FIELDS = ["fwd", "stats_rows", "dgrad", "wgrad", "ws_wgrad"]
DTYPES = [BF16, F16]
ALLOWS = [ALL, ALL & ~FUSED, ALL & ~STATS, ALL & ~WGRAD, ALL & ~BACKWARD, ALL & ~DGRAD_ACC, 0]
SHAPES = [(2, 2, 5, 5, 7), (2, 2, 7, 7, 13), (17, 6, 7, 7, 13), (5, 7, 14, 14, 47), (4, 3, 12, 10, 9), (9, 2, 28, 28, 49), (7, 2, 28, 20, 13),
          (3, 2, 32, 32, 31), (3, 2, 56, 56, 51), (2, 2, 34, 64, 31), (2, 2, 48, 40, 31), (2, 2, 62, 56, 51), (3, 2, 96, 96, 61), (2, 2, 80, 96, 33),
          (2, 2, 112, 112, 51), (128, 96, 56, 56, 51), (128, 192, 28, 28, 49), (128, 384, 14, 14, 47), (128, 768, 7, 7, 13)]      # (N, C, H, W, K)
GRID = [(dt,) + shape + (allow,) for dt in DTYPES for shape in SHAPES for allow in ALLOWS]
SWITCHES = [("SLAK_TRI_ROWS", "0"), ("SLAK_TRI_WAVE", "0"), ("SLAK_SMALL_TRI_BWD", "0"), ("SLAK_WGRAD_REDUCE", "1")]     # each in a process of its own


def load(path):
    L = ctypes.CDLL(path)
    for name in ("slak_dwconv2d_tri_filter_workspace_bytes", "slak_dwconv2d_pair_filter_workspace_bytes"):
        getattr(L, name).restype = ctypes.c_size_t
    return L


def ladder(L, dt, N, C, H, W, K, allow):
    """One row of FIELDS: the first rung of every step, in the order of the header's table, that the library supports and `allow` admits."""
    shape = (dt, N, C, H, W, K)
    fused, stats, wgrad_ok = bool(allow & FUSED), bool(allow & STATS), bool(allow & WGRAD)
    tri_bytes = L.slak_dwconv2d_tri_filter_workspace_bytes(*shape)
    srows = 0
    if fused and L.slak_dwconv2d_tri_supported_op(*shape, 0) == 1:
        srows = max(L.slak_dwconv2d_tri_stats_rows(*shape), 0) if stats else 0
        fwd = FWD_TRI_STATS if srows > 0 else FWD_TRI
    else:
        fwd = FWD_BRANCH_STATS if stats else FWD_BRANCH
    if fused and wgrad_ok and (allow & BACKWARD) and tri_bytes > 0 and L.slak_dwconv2d_tri_backward_supported(*shape) == 1:
        return [fwd, srows, DGRAD_ONE, WGRAD_ONE, tri_bytes]
    if fused and L.slak_dwconv2d_tri_supported_op(*shape, 1) == 1:
        dgrad = DGRAD_TRI
    else:
        dgrad = DGRAD_BRANCH_ACC if allow & DGRAD_ACC else DGRAD_BRANCH_ADD
    wgrad, ws = WGRAD_BRANCH, 0
    if wgrad_ok and tri_bytes > 0:
        wgrad, ws = WGRAD_TRI, tri_bytes
    elif wgrad_ok:
        pair_bytes = L.slak_dwconv2d_pair_filter_workspace_bytes(*shape)
        if pair_bytes > 0:
            wgrad, ws = WGRAD_PAIR, pair_bytes
    return [int(v) for v in (fwd, srows, dgrad, wgrad, ws)]


def rows(lib_path):
    L = load(lib_path)
    return [ladder(L, *point) for point in GRID]


def in_child(script, switch, value, *args):
    """What `script --rows ARGS` prints (JSON) in a fresh process with `switch`=`value`."""
    env = dict(os.environ)
    env[switch] = value
    return json.loads(subprocess.run([sys.executable, script, "--rows"] + list(args), env=env, check=True, stdout=subprocess.PIPE).stdout)


def dumps(doc):
    """One grid point per line."""
    head = {k: v for k, v in doc.items() if k != "rows"}
    body = ",\n".join('  "%s": [\n%s\n  ]' % (name, ",\n".join("    " + json.dumps(r) for r in rs)) for name, rs in doc["rows"].items())
    return json.dumps(head)[:-1] + ', "rows": {\n' + body + "\n}}\n"


if __name__ == "__main__":
    arg = lambda flag, default: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default
    lib_path = os.path.abspath(arg("--lib", DEFAULT_LIB))
    if "--rows" in sys.argv:
        print(json.dumps(rows(lib_path)))
    else:
        doc = {"fields": FIELDS, "grid": "(dtype, N, C, H, W, K, allow) for dtype in dtype for (N, C, H, W, K) in shape for allow in allow",
               "dtype": DTYPES, "shape": [list(s) for s in SHAPES], "allow": ALLOWS, "rows": {"default": rows(lib_path)}}
        for name, value in SWITCHES:
            doc["rows"]["%s=%s" % (name, value)] = in_child(os.path.abspath(__file__), name, value, "--lib", lib_path)
        with open(arg("--out", os.path.join(HERE, "tri_plan.json")), "w") as f:
            f.write(dumps(doc))
