"""Dev: what the C ABI decides for a depthwise-conv call.

    python tools/print_dispatch.py                    which kernel family every (config, stage, branch, op) of the BASELINE configurations lands on
                                                      (slak_debug_last_kernel; needs the GPU) -> tests/golden/dispatch_table.json
    python tools/print_dispatch.py --small            the same for the small shapes the parity tests launch -> tests/golden/dispatch_table_small.json
    python tools/print_dispatch.py --queries OUT.npz  the support / size queries (host code only, no GPU needed) over QUERY_GRID, and over the stage
                                                      shapes with each switch of QUERY_SWITCHES off -> tests/golden/dispatch_queries.npz
    python tools/print_dispatch.py --mlp              slak_mlp_plan for the pointwise MLP of every stage of the configurations (host code only)
    python tools/print_dispatch.py --tri              slak_tri_plan for the three branch convs of every stage of the configurations (host code only)
    python tools/print_dispatch.py --stage-queries    (what --queries runs in a child process per switch: switches are read once per process)
    python tools/print_dispatch.py --switches OUT.json  the launches of the small shapes (--small) in one child process per conv A/B switch
                                                      of tests/ab_switches.py's SWITCHES, the switch at its flip value: per switch the keys whose family differs from
                                                      dispatch_table_small.json (needs the GPU; without one that part of OUT.json is kept as it is); per block-tail switch what
                                                      slak_block_tail_family answers in a DEFAULT process on the switch's shapes (host code) -> tests/golden/dispatch_table_switches.json

tests/test_dispatch_gpu.py and tests/test_dispatch_queries.py load table(), small_shapes(), queries() from this file by path."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 2
CONFIGS = {"cfg1_slak_t_224": (128, [(96, 56, 51), (192, 28, 49), (384, 14, 47), (768, 7, 13)]),
           "cfg3_slak_b_224": (64, [(128, 56, 51), (256, 28, 49), (512, 14, 47), (1024, 7, 13)]),
           "cfg4_slak_t_384": (64, [(96, 96, 61), (192, 48, 59), (384, 24, 57), (768, 12, 13)])}


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def benchmark_shapes():
    """A shape set: (blocks, convs).  blocks: (key, N, C, H, W, K) in bf16 -- the per-branch entry points at K x 5, 5 x K and 5 x 5, then the
    three-branch and pair entry points where their queries say yes; convs: (key, dtype, N, C, H, W, kh, kw) -- the per-branch entry points only."""
    return [("%s/s%d" % (cfg, si + 1), N, C, HW, HW, K) for cfg, (N, stages) in CONFIGS.items() for si, (C, HW, K) in enumerate(stages)], []


def small_shapes():
    """Only shapes the parity tests already launch (no kernel meets a shape here that it has not met there)."""
    for p in (os.path.join(ROOT, "tests"), ROOT):    # the test modules import the oracle package and their shared helpers (tests/conv_calls.py)
        if p not in sys.path:
            sys.path.insert(0, p)
    fused, mfma = _load("tests/test_fused_launches_gpu.py", "_fused_shapes"), _load("tests/test_mfma_gpu.py", "_mfma_shapes")
    blocks = fused.TRI_SMALL + fused.TRI_WIDE + fused.TRI_BWD + fused.TRI_WAVE + fused.PAIR_SMALL + [s for s in fused.TRI_ROWS if s[0] <= 9]
    blocks = [("n%d_c%d_%dx%d_k%d" % s,) + s for s in dict.fromkeys(blocks)]
    convs = [("n%d_c%d_%dx%d_%dx%d/%s" % (s + (name,)), dt) + s for s in mfma.SHAPES for name, dt in (("bf16", BF16), ("f32", F32))]
    return blocks, convs


def table(dev, shapes):
    """{key: kernel family} of every launch of the shape set, as slak_debug_last_kernel() reports it."""
    import torch
    from slak_amd import _lib
    L = _lib.lib(); st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    def last(): return L.slak_debug_last_kernel().decode()
    out = {}

    def per_branch(key, dt, N, C, H, W, kh, kw):
        x = torch.randn(N, C, H, W, device=dev).to(torch.bfloat16 if dt == BF16 else torch.float32); y = torch.empty_like(x)
        w = torch.randn(C, 1, kh, kw, device=dev) * 0.02; dw = torch.empty_like(w)
        dims = (N, C, H, W, kh, kw)
        nb = max(int(L.slak_dwconv2d_workspace_bytes(op, *dims, dt)) for op in (0, 1, 2)); ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        _lib.check(L.slak_dwconv2d_forward(x.data_ptr(), dt, w.data_ptr(), 0, y.data_ptr(), dt, *dims, ws.data_ptr(), ws.numel(), st)); out[key + "/fwd"] = last()
        _lib.check(L.slak_dwconv2d_backward_data(x.data_ptr(), dt, w.data_ptr(), 0, y.data_ptr(), dt, *dims, ws.data_ptr(), ws.numel(), st)); out[key + "/bwd_data"] = last()
        rc = L.slak_dwconv2d_backward_data_accumulate(x.data_ptr(), dt, w.data_ptr(), 0, y.data_ptr(), dt, *dims, ws.data_ptr(), ws.numel(), st); out[key + "/bwd_data_acc"] = last() if rc == 0 else "unsupported"
        _lib.check(L.slak_dwconv2d_backward_filter(x.data_ptr(), dt, x.data_ptr(), dt, dw.data_ptr(), *dims, ws.data_ptr(), ws.numel(), st)); out[key + "/bwd_filter"] = last()

    blocks, convs = shapes
    for prefix, N, C, H, W, K in blocks:
        dt = BF16
        for kh, kw in ((K, 5), (5, K), (5, 5)):
            per_branch("%s/%dx%d" % (prefix, kh, kw), dt, N, C, H, W, kh, kw)
        x = torch.randn(N, C, H, W, device=dev).bfloat16()
        key = prefix + "/tri"
        out[key + "/use_fwd"] = int(L.slak_dwconv2d_tri_supported_op(dt, N, C, H, W, K, 0)); out[key + "/use_bwd_data"] = int(L.slak_dwconv2d_tri_supported_op(dt, N, C, H, W, K, 1))
        wts = [torch.randn(C, 1, kh, kw, device=dev) * 0.02 for kh, kw in ((K, 5), (5, K), (5, 5))]; ys = [torch.empty_like(x) for _ in range(3)]
        if out[key + "/use_fwd"]:
            _lib.check(L.slak_dwconv2d_tri_forward(x.data_ptr(), wts[0].data_ptr(), wts[1].data_ptr(), wts[2].data_ptr(), ys[0].data_ptr(), ys[1].data_ptr(), ys[2].data_ptr(), dt, N, C, H, W, K, st)); out[key + "/fwd"] = last()
        if out[key + "/use_bwd_data"]:
            _lib.check(L.slak_dwconv2d_tri_backward_data(x.data_ptr(), ys[0].data_ptr(), ys[1].data_ptr(), wts[0].data_ptr(), wts[1].data_ptr(), wts[2].data_ptr(), ys[2].data_ptr(), dt, N, C, H, W, K, st)); out[key + "/bwd_data"] = last()
        nb = int(L.slak_dwconv2d_tri_filter_workspace_bytes(dt, N, C, H, W, K))
        if nb:
            ws = torch.empty(nb, dtype=torch.uint8, device=dev); dws = [torch.empty_like(w) for w in wts]
            _lib.check(L.slak_dwconv2d_tri_backward_filter(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), dws[0].data_ptr(), dws[1].data_ptr(), dws[2].data_ptr(), dt, N, C, H, W, K, ws.data_ptr(), nb, st)); out[key + "/bwd_filter"] = last()
        out[key + "/use_bwd"] = int(L.slak_dwconv2d_tri_backward_supported(dt, N, C, H, W, K))     # data gradient + the three weight gradients in one launch
        if out[key + "/use_bwd"]:
            _lib.check(L.slak_dwconv2d_tri_backward(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), wts[0].data_ptr(), wts[1].data_ptr(), wts[2].data_ptr(), ys[2].data_ptr(), dws[0].data_ptr(), dws[1].data_ptr(), dws[2].data_ptr(), dt, N, C, H, W, K, ws.data_ptr(), nb, st)); out[key + "/bwd"] = last()
        nb = int(L.slak_dwconv2d_pair_filter_workspace_bytes(dt, N, C, H, W, K))
        if nb:
            ws = torch.empty(nb, dtype=torch.uint8, device=dev); dws = [torch.empty_like(wts[0]), torch.empty_like(wts[2])]
            rc = L.slak_dwconv2d_pair_backward_filter(x.data_ptr(), x.data_ptr(), x.data_ptr(), dws[0].data_ptr(), dws[1].data_ptr(), dt, N, C, H, W, K, ws.data_ptr(), nb, st)
            out[prefix + "/pair/bwd_filter"] = last() if rc == 0 else "unsupported"
    for key, dt, N, C, H, W, kh, kw in convs:
        per_branch(key, dt, N, C, H, W, kh, kw)
    torch.cuda.synchronize()
    return out


# ---- the support and size queries: pure host code (the CU count falls back to the MI355X's 256 without a device) ----
QUERY_GRID = [(dt, N, C, H, W, K) for dt in (F32, F16, BF16) for N, C in ((2, 3), (64, 96), (128, 768), (1, 1030))
              for H in (7, 8, 12, 14, 15, 16, 17, 24, 28, 32, 33, 36, 40, 48, 56, 62, 64, 65, 80, 96, 97, 112) for W in dict.fromkeys((H, max(7, H - 8)))
              for K in (5, 7, 13, 31, 51, 61, 63)]
STAGE_POINTS = [(BF16, N, C, HW, HW, K) for N, stages in CONFIGS.values() for C, HW, K in stages]
QUERY_SWITCHES = ["SLAK_STREAM_TRI", "SLAK_TEAM_TRI", "SLAK_WIDE_TRI", "SLAK_SMALL_QUAD", "SLAK_SMALL_TRI_BWD", "SLAK_TRI_ROWS", "SLAK_TRI_WAVE",
                  "SLAK_MFMA_VROWS", "SLAK_VROWS_PAIR", "SLAK_MFMA_VWAVE", "SLAK_MFMA_HWAVE"]
QUERY_COLUMNS = 16      # tri_supported_op 0 / 1, tri_supported, tri_stats_rows, tri / pair filter workspace, tri_backward_supported, workspace_bytes 3 ops x 3 filters


def queries(L, points):
    """One row of QUERY_COLUMNS integers per (dtype, N, C, H, W, K).  L: the ctypes library (slak_amd/_lib.py's lib())."""
    rows = []
    for dt, N, C, H, W, K in points:
        s = (dt, N, C, H, W, K)
        row = [L.slak_dwconv2d_tri_supported_op(*s, 0), L.slak_dwconv2d_tri_supported_op(*s, 1), L.slak_dwconv2d_tri_supported(*s), L.slak_dwconv2d_tri_stats_rows(*s),
               L.slak_dwconv2d_tri_filter_workspace_bytes(*s), L.slak_dwconv2d_pair_filter_workspace_bytes(*s), L.slak_dwconv2d_tri_backward_supported(*s)]
        row += [L.slak_dwconv2d_workspace_bytes(op, N, C, H, W, kh, kw, dt) for kh, kw in ((K, 5), (5, K), (5, 5)) for op in (0, 1, 2)]
        rows.append([int(v) for v in row])
    return rows


def load_lib():
    """The ctypes binding without importing the package (and torch with it): the query mode is host code only."""
    return _load("slak_amd/_lib.py", "_slak_lib_only").lib()


def stage_queries_with_switch_off(name):
    """queries(STAGE_POINTS) as a fresh process with `name`=0 answers them."""
    env = dict(os.environ); env[name] = "0"
    return json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--stage-queries"], env=env, check=True, stdout=subprocess.PIPE).stdout)


def all_queries():
    """{array name: rows}: what tests/golden/dispatch_queries.npz holds."""
    out = {"grid": queries(load_lib(), QUERY_GRID)}
    for name in QUERY_SWITCHES:
        out[name] = stage_queries_with_switch_off(name)
    return out


def switch_tables(path):
    """What tests/golden/dispatch_table_switches.json holds: {conv switch: {key: family}} over the keys of table(small_shapes()) whose family a process with
    the switch flipped (SWITCHES' flip value: "1" for a default-off switch) reports differently from tests/golden/dispatch_table_small.json (None: the launch is
    gone), and {block-tail switch: {shape: {op: family}}} as a DEFAULT process answers."""
    ab = _load("tests/ab_switches.py", "_ab_switches")
    out = json.load(open(path)) if os.path.exists(path) else {}
    lib = _load("slak_amd/_lib.py", "_slak_lib_only")
    for name, sw in ab.SWITCHES.items():
        assert name not in os.environ, name + " is set: the default answers need a default process"
        if sw["group"] == "tail":
            out[name] = {ab.tail_key(c): ab.tail_families(lib.lib(), lib, c) for c in sw["cases"]}
    import torch
    if torch.cuda.is_available():
        small = json.load(open(os.path.join(ROOT, "tests", "golden", "dispatch_table_small.json")))
        for name in ab.CONV_SWITCHES:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--small"], env=dict(os.environ, **{name: ab.SWITCHES[name]["flip"]}), check=True,
                               stdout=subprocess.PIPE, timeout=300)
            out[name] = ab.table_diff(small, json.loads(r.stdout))
            print(name, len(out[name]), "keys differ", file=sys.stderr)
    else:
        print("no GPU: the conv switches' tables are left as they are", file=sys.stderr)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


def mlp_plans():
    """{stage: {step: rung}}: slak_mlp_plan (allow = every kernel family) for the pointwise MLP of every stage of CONFIGS.  Host code only."""
    lib = _load("slak_amd/_lib.py", "_slak_lib_only")
    L, out = lib.lib(), {}
    for cfg, (N, stages) in CONFIGS.items():
        for si, (C, HW, _) in enumerate(stages):
            p = lib.MlpPlan()
            lib.check(L.slak_mlp_plan(N * HW * HW, 4 * C, C, lib.MLP_ALLOW_ALL, ctypes.byref(p)), "slak_mlp_plan")
            out["%s/s%d" % (cfg, si + 1)] = dict({f: lib.MLP_RUNG_NAMES[getattr(p, f)] for f in ("pw1", "pw2", "dy1", "dt", "dw1", "dw2")}, splits=p.splits)
    return out


def tri_plans():
    """{stage: {step: rung}}: slak_tri_plan (allow = every launch, bf16) for the three branch convs of every stage of CONFIGS.  Host code only."""
    lib = _load("slak_amd/_lib.py", "_slak_lib_only")
    L, out = lib.lib(), {}
    for cfg, (N, stages) in CONFIGS.items():
        for si, (C, HW, K) in enumerate(stages):
            p = lib.TriPlan()
            lib.check(L.slak_tri_plan(BF16, N, C, HW, HW, K, lib.TRI_ALLOW_ALL, ctypes.byref(p)), "slak_tri_plan")
            out["%s/s%d" % (cfg, si + 1)] = {"fwd": lib.TRI_FWD_NAMES[p.fwd], "stats_rows": p.stats_rows, "dgrad": lib.TRI_DGRAD_NAMES[p.dgrad],
                                             "wgrad": lib.TRI_WGRAD_NAMES[p.wgrad], "ws_wgrad": p.ws_wgrad}
    return out


if __name__ == "__main__":
    if "--mlp" in sys.argv:
        print(json.dumps(mlp_plans(), indent=0))
    elif "--tri" in sys.argv:
        print(json.dumps(tri_plans(), indent=0))
    elif "--switches" in sys.argv:
        switch_tables(sys.argv[sys.argv.index("--switches") + 1])
    elif "--stage-queries" in sys.argv:
        print(json.dumps(queries(load_lib(), STAGE_POINTS)))
    elif "--queries" in sys.argv:
        import numpy as np
        np.savez_compressed(sys.argv[sys.argv.index("--queries") + 1], **{k: np.asarray(v, dtype=np.int64) for k, v in all_queries().items()})
    else:
        sys.path.insert(0, ROOT)
        import torch
        print(json.dumps(table(torch.device("cuda:0"), small_shapes() if "--small" in sys.argv else benchmark_shapes()), indent=0))
