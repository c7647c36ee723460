"""The shipped A/B switches (slak_env_flag() call sites of slak_amd/csrc/) and what a process started with one of them flipped has to show.

SWITCHES is the inventory: tests/test_ab_switches_cpu.py holds it against the call sites, tests/test_ab_switches_gpu.py starts

    python tests/ab_switches.py NAME          (with NAME=<flip> in the environment: a switch is read once per process)

per switch and asserts on the one JSON document this file prints.  Per switch the child
  (a) proves that the flag changed what runs: the launches' kernel families (tools/print_dispatch.py's table against
      tests/golden/dispatch_table_switches.json), slak_block_tail_family, or slak_mlp_plan and the *_supported queries;
  (b) runs the affected entry points on the switch's shapes against the checker the default-path tests use (the C oracle on the rounded operands,
      fp64 torch) with THEIR bounds -- never against the default kernel;
  (c) records every launch that refused although its size / support query had said yes ("violations").
Nothing here imports torch at module level: the inventory test runs without a GPU."""
import ctypes
import importlib.util
import json
import math
import os
import sys
import time

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
PINNED = os.path.join(TESTS, "golden", "dispatch_table_switches.json")


def _sw(group, cases, default=True, no_observable=False, covered_by=None):
    return {"group": group, "default": default, "flip": "0" if default else "1", "cases": cases, "no_observable": no_observable, "covered_by": covered_by}


# conv cases: (N, C, H, W, K) = a block shape (the per-branch entry points at K x 5, 5 x K and 5 x 5, then the three-branch, pair and one-launch-backward
# entry points where their queries say yes); (N, C, H, W, kh, kw) = one per-branch shape.  At most three per switch, the smallest of the parity
# tests' shapes whose family the switch changes (the four diagonal-tile shapes of TRI_ROWS for SLAK_TRI_ROWS_SD, whose family name stays).
_S56 = [(3, 2, 56, 56, 51), (2, 2, 34, 64, 31), (2, 2, 62, 56, 51)]
_S28 = [(9, 2, 28, 28, 49), (7, 2, 28, 20, 13), (3, 2, 32, 32, 31)]
# tail cases: (N, C, H, W) at N = 2, from tests/test_block_tail_gpu.py's lists; pointwise cases: (M, Cp) with the rungs slak_mlp_plan must answer
# in the flipped process ("expect") and answers in a default one ("default", held by the CPU test)
SWITCHES = {
    "SLAK_MFMA_DMA": _sw("conv", [(3, 2, 56, 56, 51), (9, 2, 28, 28, 49), (5, 4, 24, 28, 5, 31)]),
    "SLAK_MFMA_SMALL": _sw("conv", [(17, 6, 7, 7, 13), (6, 5, 7, 7, 13), (1, 1, 7, 7, 13, 5)]),       # (only planes up to 7 x 7 reach the channel-blocked kernel)
    "SLAK_MFMA_SMALL_DMA": _sw("conv", [(5, 7, 14, 14, 47), (4, 3, 12, 10, 9), (9, 4, 12, 12, 13)]),
    "SLAK_MFMA_VROWS": _sw("conv", _S56),
    "SLAK_VROWS_PAIR": _sw("conv", _S56),
    "SLAK_MFMA_VWAVE": _sw("conv", _S28),
    "SLAK_MFMA_HWAVE": _sw("conv", _S28),
    "SLAK_WGRAD_REDUCE": _sw("conv", [(3, 2, 56, 56, 51), (9, 2, 28, 28, 49), (5, 7, 14, 14, 47)], default=False),
    "SLAK_STREAM_TRI": _sw("conv", [(3, 2, 56, 56, 51), (2, 2, 48, 40, 31), (3, 2, 48, 48, 59)]),
    "SLAK_TEAM_TRI": _sw("conv", _S28),
    "SLAK_WIDE_TRI": _sw("conv", [(3, 2, 96, 96, 61), (2, 2, 80, 96, 33)]),
    # the quad kernels keep the family name of the kernels they replace on 7 x 7: no launch of the table changes; slak_dwconv2d_tri_stats_rows does
    # (the one-plane-per-tile kernel gathers no statistics there): {case: (default process, flipped process)}
    "SLAK_SMALL_QUAD": dict(_sw("conv", [(17, 6, 7, 7, 13), (6, 5, 7, 7, 13)], no_observable=True), stats_rows={(17, 6, 7, 7, 13): (3, 0), (6, 5, 7, 7, 13): (1, 0)}),
    "SLAK_SMALL_TRI_BWD": _sw("conv", [(5, 7, 14, 14, 47), (4, 3, 12, 10, 9), (9, 4, 12, 12, 13)]),
    "SLAK_TRI_ROWS": _sw("conv", _S56),
    "SLAK_TRI_ROWS_SD": _sw("conv", [(3, 2, 40, 56, 27), (2, 2, 34, 64, 31), (2, 2, 62, 56, 51), (5, 2, 50, 56, 9)], no_observable=True),
    "SLAK_TRI_WAVE": _sw("conv", _S28),
    "SLAK_TAIL_REG": _sw("tail", [(2, 96, 16, 16), (2, 384, 14, 14), (2, 768, 7, 7)]),
    "SLAK_RT_CHAN": _sw("tail", [(2, 96, 16, 16), (2, 384, 14, 14), (2, 768, 7, 7)]),
    "SLAK_RT_WIDE": _sw("tail", [(2, 384, 20, 20), (2, 384, 14, 14)], no_observable=True),   # 20 x 20: the register family, whose fp32 residual forward the switch changes
    "SLAK_LN_CF_REG": _sw("ln_cf", [(2, 96, 28, 28), (2, 192, 28, 28), (2, 128, 9, 11)], no_observable=True),
    "SLAK_LINEAR_GEMM": _sw("pointwise", [{"M": 777, "C": 192, "expect": {"pw1": "library", "dy1": "library"}, "default": {"pw1": "gemm", "dy1": "gemm"}}]),
    "SLAK_LINEAR_MLP_FWD": _sw("pointwise", [{"M": 96, "C": 96, "expect": {"pw1": "nt"}, "default": {"pw1": "fused"}},
                                             {"M": 401, "C": 96, "expect": {"pw1": "nt"}, "default": {"pw1": "fused"}}]),
    "SLAK_LINEAR_GELU_BWD": _sw("pointwise", [{"M": 96, "C": 96, "expect": {"dy1": "nt"}, "default": {"dy1": "fused_dt"}},
                                              {"M": 416, "C": 96, "expect": {"dy1": "nt"}, "default": {"dy1": "fused_dt"}}]),
    "SLAK_LINEAR_GELU_BWD_DT": _sw("pointwise", [{"M": 96, "C": 96, "expect": {"dy1": "fused"}, "default": {"dy1": "fused_dt"}},
                                                 {"M": 416, "C": 96, "expect": {"dy1": "fused"}, "default": {"dy1": "fused_dt"}}]),
    # ("wgrad": further (N1, N2) of slak_linear_wgrad at the case's M -- the two smallest M >= 32 entries of test_linear_skinny_gpu.py's WGRAD_SHAPES on the 128 x 64 tiles)
    "SLAK_LINEAR_WGRAD_128": _sw("pointwise", [{"M": 40, "C": 128, "expect": {"dw1": "library", "dw2": "library"}, "default": {"dw1": "kernel", "dw2": "kernel"}, "wgrad": [(128, 256)]},
                                               {"M": 1000, "C": 256, "expect": {"dw1": "library", "dw2": "library"}, "default": {"dw1": "kernel", "dw2": "kernel"},
                                                "wgrad": [(256, 1024)]}]),
    "SLAK_FP32_MFMA": _sw(None, [], default=False, covered_by="tests/test_fp32_mfma_gpu.py through its setter (slak_set_fp32_matrix_cores)"),
}
CASE_SWITCHES = [n for n, s in SWITCHES.items() if not s["covered_by"]]
CONV_SWITCHES = [n for n in CASE_SWITCHES if SWITCHES[n]["group"] == "conv"]
TAIL_OPS = (("ln_fwd", 0, 0), ("ln_bwd", 1, 0), ("sr_fwd/f32", 2, 0), ("sr_fwd/bf16", 2, 2), ("sr_bwd", 3, 0))     # (name, SLAK_TAIL_* op, shortcut dtype)


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def table_diff(base, got):
    """{key: family in `got`, None where the key is gone} over the keys on which the two tables differ."""
    return {k: got.get(k) for k in sorted(set(base) | set(got)) if base.get(k) != got.get(k)}


def case_keys(case):
    """The dispatch-table key prefix of a conv case."""
    return ("n%d_c%d_%dx%d_k%d/" % case) if len(case) == 5 else ("n%d_c%d_%dx%d_%dx%d/bf16/" % case)


def tail_families(L, lib, case):
    N, C, H, W = case
    return {name: lib.TAIL_FAMILY_NAMES[L.slak_block_tail_family(op, dt, N, C, H * W, C)] for name, op, dt in TAIL_OPS}


def mlp_rungs(L, lib, M, C):
    p = lib.MlpPlan()
    lib.check(L.slak_mlp_plan(M, 4 * C, C, lib.MLP_ALLOW_ALL, ctypes.byref(p)), "slak_mlp_plan")
    return {f: lib.MLP_RUNG_NAMES[getattr(p, f)] for f in ("pw1", "pw2", "dy1", "dt", "dw1", "dw2")}


def tail_key(case):
    return "n%d_c%d_%dx%d" % case


# ------------------------------------------------------------------------------------------------ the child
class _Declined(Exception):
    pass


class _Doc:
    def __init__(self, name):
        self.d = {"switch": name, "flip": SWITCHES[name]["flip"], "observable": {}, "checks": [], "violations": []}

    def check(self, what, ran, fn):
        """fn() -> the largest error; an AssertionError is a missed bound, a SlakHipError a launch that failed after its query had said yes"""
        from slak_amd import _lib
        e = {"what": what, "ran": ran() if callable(ran) else ran}
        try:
            e["err"] = float(fn())
            e["ok"] = True
            if callable(ran):
                e["ran"] = ran()
        except _Declined as ex:
            e["ok"], e["err"], e["ran"] = True, None, str(ex)
        except AssertionError as ex:
            e["ok"], e["msg"] = False, str(ex)[:400]
        except _lib.SlakHipError as ex:
            e["ok"], e["msg"] = False, str(ex)[:400]
            self.d["violations"].append("%s: %s" % (what, str(ex)[:200]))
        self.d["checks"].append(e)

    def declined(self, what):
        self.d["checks"].append({"what": what, "ran": "declined (the query answers 0)", "ok": True, "err": None})


def _last():
    from slak_amd import _lib
    return _lib.lib().slak_debug_last_kernel().decode()


def _maxerr(got, ref):
    import numpy as np
    return float(np.abs(got.detach().double().cpu().numpy() - ref).max())


def _conv_child(doc, name, dev):
    import numpy as np
    import torch
    import oracle
    from slak_amd import _lib, ops
    from conv_calls import _check_dw, _check_lowp, _dt, _filters, _pair_wgrad, _r, _tri_bwd, _tri_dgrad, _tri_fwd, _tri_wgrad
    sw = SWITCHES[name]
    L = _lib.lib()
    tool = load("tools/print_dispatch.py", "_print_dispatch")
    pinned = json.load(open(PINNED))
    base = json.load(open(os.path.join(TESTS, "golden", "dispatch_table_small.json")))
    diff = table_diff(base, tool.table(dev, tool.small_shapes()))
    obs = doc.d["observable"]
    obs["changed_keys"] = len(diff)
    obs["families"] = sorted(set(str(v) for v in diff.values()))
    obs["matches_pinned"] = diff == pinned[name]
    if not obs["matches_pinned"]:
        obs["not_as_pinned"] = {k: (diff.get(k, "(unchanged)"), pinned[name].get(k, "(unchanged)")) for k in sorted(set(diff) | set(pinned[name]))
                                if diff.get(k, 0) != pinned[name].get(k, 0)}
    if "stats_rows" in sw:                                  # bf16: the statistics rows the three-branch forward would leave
        obs["stats_rows"] = {case_keys(c): int(L.slak_dwconv2d_tri_stats_rows(_lib.SLAK_BF16, *c)) for c in sw["stats_rows"]}
        obs["stats_rows_as_expected"] = all(obs["stats_rows"][case_keys(c)] == flipped for c, (_, flipped) in sw["stats_rows"].items())
    obs["cases_changed"] = {case_keys(c): sum(k.startswith(case_keys(c)) for k in diff) for c in sw["cases"]}

    def branch_wgrad_bound(dw, ref, n_terms):              # tests/test_mfma_gpu.py::test_mfma_forward_dgrad_wgrad_vs_oracle: fp32 accumulation only
        err = np.abs(dw.double().cpu().numpy() - ref).max()
        assert err <= 1e-5 * max(1.0, np.abs(ref).max()) * max(1.0, n_terms ** 0.5 / 30), err
        return err

    def two_roundings(got, ref, parts, dtype, acc=5e-6):    # tests/test_fused_launches_gpu.py: each branch's partial may be rounded before the sum is
        ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
        got = got.detach().double().cpu().numpy()
        scale = max(1.0, float(np.abs(ref).max()))
        assert np.abs(got - ref).max() <= 1e-2 * scale
        bound = ulp * (np.abs(ref) + sum(np.abs(p) for p in parts)) + acc * scale
        assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) - bound).max())
        return np.abs(got - ref).max()

    def per_branch(tag, x, dy, base_dx, w, dtype, refs):
        """the four per-branch entry points on one filter; refs = (y, dx, dw) of the oracle on the rounded operands"""
        N, C, H, W = x.shape
        def lowp(got, ref, what):
            _check_lowp(got, ref, dtype, what)
            return _maxerr(got, ref)
        doc.check(tag + "/fwd", _last, lambda: lowp(ops.dwconv2d_forward(x, w), refs[0], "fwd"))
        doc.check(tag + "/bwd_data", _last, lambda: lowp(ops.dwconv2d_backward_data(dy, w), refs[1], "dgrad"))

        def acc():
            # dx = fl(b + fl(g)), a tensor add of two low-precision tensors: |dx - (b + g)| <= u |b + fl(g)| + u |g| <= u |b + g| + (u + u^2) |g| with u
            # half an output ulp, + the accumulation term of the data-gradient bound
            ws_nb = int(L.slak_dwconv2d_workspace_bytes(_lib.OP_BWD_DATA, N, C, H, W, w.shape[2], w.shape[3], _dt(dtype)))
            wsb = torch.empty(max(ws_nb, 16), dtype=torch.uint8, device=dev)
            dx = base_dx.clone()
            rc = L.slak_dwconv2d_backward_data_accumulate(dy.data_ptr(), _dt(dtype), w.data_ptr(), _lib.SLAK_F32, dx.data_ptr(), _dt(dtype), N, C, H, W,
                                                          w.shape[2], w.shape[3], wsb.data_ptr(), ws_nb, torch.cuda.current_stream(dev).cuda_stream)
            if rc == _lib.ERR_UNSUPPORTED:                  # no query of its own: UNSUPPORTED is the documented answer of every kernel but the ring kernel
                raise _Declined("unsupported (no accumulating kernel for the shape: the caller adds)")
            _lib.check(rc, "slak_dwconv2d_backward_data_accumulate")
            ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
            ref = base_dx.double().cpu().numpy() + refs[1]
            e = np.abs(dx.double().cpu().numpy() - ref)
            bound = ulp * np.abs(ref) + (ulp + ulp * ulp) * np.abs(refs[1]) + 5e-6 * max(1.0, float(np.abs(ref).max()))
            assert (e <= bound).all(), float((e - bound).max())
            return e.max()
        doc.check(tag + "/bwd_data_acc", _last, acc)
        doc.check(tag + "/bwd_filter", _last, lambda: branch_wgrad_bound(ops.dwconv2d_backward_filter(dy, x, w), refs[2], N * H * W))

    for dtype in (torch.bfloat16, torch.float16):
        dn = "bf16" if dtype == torch.bfloat16 else "f16"
        dt = _dt(dtype)
        for case in sw["cases"]:
            tag0 = case_keys(case).replace("/bf16/", "/") + dn
            torch.manual_seed(sum(case))
            N, C, H, W = case[:4]
            x = torch.randn(N, C, H, W, device=dev).to(dtype)
            base_dx = torch.randn(N, C, H, W, device=dev).to(dtype)
            xr = _r(x, dtype)
            if len(case) == 6:
                kh, kw = case[4:]
                dy = torch.randn(N, C, H, W, device=dev).to(dtype)
                w = torch.randn(C, 1, kh, kw, device=dev) * 0.05
                wr, dyr = _r(w, dtype), _r(dy, dtype)
                per_branch(tag0, x, dy, base_dx, w, dtype, (oracle.dwconv2d_fwd(xr, wr), oracle.dwconv2d_bwd_data(dyr, wr), oracle.dwconv2d_bwd_filter(dyr, xr, kh, kw)))
                continue
            K = case[4]
            s = (dt, N, C, H, W, K)
            dys = [torch.randn(N, C, H, W, device=dev).to(dtype) for _ in range(3)]
            ws = _filters(C, K, dev, K + C)
            wr = [_r(w, dtype) for w in ws]
            dyr = [_r(d, dtype) for d in dys]
            fil = ((K, 5), (5, K), (5, 5))
            yref = [oracle.dwconv2d_fwd(xr, w) for w in wr]
            parts = [oracle.dwconv2d_bwd_data(d, w) for d, w in zip(dyr, wr)]
            dwref = [oracle.dwconv2d_bwd_filter(d, xr, kh, kw) for d, (kh, kw) in zip(dyr, fil)]
            for b, (kh, kw) in enumerate(fil):
                per_branch("%s/%dx%d" % (tag0, kh, kw), x, dys[b], base_dx, ws[b], dtype, (yref[b], parts[b], dwref[b]))
            dxref = sum(parts)
            if L.slak_dwconv2d_tri_supported_op(*s, 0):
                def tri_fwd():
                    ys, _ = _tri_fwd(x, ws, K)
                    for y, r, n in zip(ys, yref, ("Kx5", "5xK", "5x5")):
                        _check_lowp(y, r, dtype, "tri fwd " + n)
                    return max(_maxerr(y, r) for y, r in zip(ys, yref))
                doc.check(tag0 + "/tri/fwd", _last, tri_fwd)
            else:
                doc.declined(tag0 + "/tri/fwd")
            if L.slak_dwconv2d_tri_stats_rows(*s) > 0:      # the forward that also leaves the branch BatchNorms' batch sums (test_tri_launches_at_bench_shapes)
                def tri_fwd_stats():
                    ys, st = _tri_fwd(x, ws, K, stats=True)
                    for y, r, n in zip(ys, yref, ("Kx5", "5xK", "5x5")):
                        _check_lowp(y, r, dtype, "tri fwd (stats) " + n)
                    sums = st.double().sum(dim=0)
                    for b, y in enumerate(ys):              # sums of the STORED outputs
                        yd = y.double()
                        s1, s2 = yd.sum(dim=(0, 2, 3)), (yd * yd).sum(dim=(0, 2, 3))
                        assert (sums[:, 2 * b] - s1).abs().max().item() <= 1e-4 * max(1.0, s2.max().item() ** 0.5 * (N * H * W) ** 0.5), "sum y, branch %d" % b
                        assert (sums[:, 2 * b + 1] - s2).abs().max().item() <= 1e-4 * s2.max().item(), "sum y^2, branch %d" % b
                    return max(_maxerr(y, r) for y, r in zip(ys, yref))
                doc.check(tag0 + "/tri/fwd_stats", _last, tri_fwd_stats)
            else:
                doc.declined(tag0 + "/tri/fwd_stats")
            if L.slak_dwconv2d_tri_supported_op(*s, 1):
                def tri_dgrad():
                    dx = _tri_dgrad(dys, ws, K)
                    if _last() == "dwconv_mfma_wide_tri":   # (test_tri_forward_and_backward_data_on_wide_maps_vs_oracle: ONE rounding)
                        return two_roundings(dx, dxref, [], dtype, acc=1e-5)
                    return two_roundings(dx, dxref, parts, dtype)
                doc.check(tag0 + "/tri/bwd_data", _last, tri_dgrad)
            else:
                doc.declined(tag0 + "/tri/bwd_data")

            def dws_vs_oracle(dws, what):
                for dw, r, (kh, kw) in zip(dws, dwref, fil):
                    _check_dw(dw, r, N * H * W, "%s dw %dx%d" % (what, kh, kw))
                return max(_maxerr(dw, r) for dw, r in zip(dws, dwref))
            if L.slak_dwconv2d_tri_filter_workspace_bytes(*s):
                doc.check(tag0 + "/tri/bwd_filter", _last, lambda: dws_vs_oracle(_tri_wgrad(dys, x, K), "tri"))
            else:
                doc.declined(tag0 + "/tri/bwd_filter")
            if L.slak_dwconv2d_tri_backward_supported(*s):
                def tri_bwd():
                    dx, dws = _tri_bwd(dys, x, ws, K)
                    return max(two_roundings(dx, dxref, parts, dtype), dws_vs_oracle(dws, "one-launch"))
                doc.check(tag0 + "/tri/bwd", _last, tri_bwd)
            else:
                doc.declined(tag0 + "/tri/bwd")
            if L.slak_dwconv2d_pair_filter_workspace_bytes(*s):
                def pair():
                    dwv, dw5 = _pair_wgrad(dys[0], dys[2], x, K)
                    _check_dw(dwv, dwref[0], N * H * W, "pair dw Kx5")
                    _check_dw(dw5, dwref[2], N * H * W, "pair dw 5x5")
                    return max(_maxerr(dwv, dwref[0]), _maxerr(dw5, dwref[2]))
                doc.check(tag0 + "/pair/bwd_filter", _last, pair)
            else:
                doc.declined(tag0 + "/pair/bwd_filter")
    torch.cuda.synchronize()


def _tail_child(doc, name, dev):
    import torch
    import torch.nn.functional as F
    from slak_amd import _lib
    from tail_calls import _close, _ln_bwd_ld, _ln_fwd_ld, _sr_bwd_ld, _sr_fwd_ld
    sw = SWITCHES[name]
    L = _lib.lib()
    pinned = json.load(open(PINNED))[name]
    obs = doc.d["observable"]
    for case in sw["cases"]:
        fam = tail_families(L, _lib, case)
        obs[tail_key(case)] = {"default": pinned[tail_key(case)], "flipped": fam, "changed": sorted(k for k in fam if fam[k] != pinned[tail_key(case)][k])}
    fam_of = lambda case, op: lambda: obs[tail_key(case)]["flipped"][op]

    def err(a, b, rel, what):
        _close(a, b, rel, what)
        return (a.double() - b.double()).abs().max().item() / max(1e-6, b.double().abs().max().item())

    for case in sw["cases"]:
        N, C, H, W = case
        tag = tail_key(case)
        torch.manual_seed(C + H)
        # test_ln_nchw_to_nhwc_matches_layer_norm: fp64 F.layer_norm on the same bf16 operands
        x = (torch.randn(N, C, H, W, device=dev) * 2 + 0.3).bfloat16()
        w = torch.randn(C, device=dev) * 0.5 + 1
        b = torch.randn(C, device=dev) * 0.1
        g = torch.randn(N, H, W, C, device=dev).bfloat16()
        xr = x.double().requires_grad_(True); wr = w.double().requires_grad_(True); br = b.double().requires_grad_(True)
        yr = F.layer_norm(xr.permute(0, 2, 3, 1), (C,), wr, br, 1e-6)
        yr.backward(g.double())
        held = {}

        def ln_fwd():
            held["ln"] = _ln_fwd_ld(L, x, w, b, None)
            return err(held["ln"][0], yr.detach(), 2.0 ** -8 * 1.01, "y")
        doc.check(tag + "/ln_fwd", fam_of(case, "ln_fwd"), ln_fwd)

        def ln_bwd():
            if "ln" not in held:
                raise AssertionError("the forward did not run")
            dx, dw, db = _ln_bwd_ld(L, g, x, w, held["ln"][1], held["ln"][2], None)
            return max(err(dx, xr.grad, 2.0 ** -8 * 1.5, "dx"), err(dw, wr.grad, 1e-4, "dweight"), err(db, br.grad, 1e-4, "dbias"))
        doc.check(tag + "/ln_bwd", fam_of(case, "ln_bwd"), ln_bwd)
        # test_scale_residual_matches_torch / _with_bf16_copy_and_second_gradient_stream: fp64 on the same operands
        torch.manual_seed(C + W)
        z = torch.randn(N, H, W, C, device=dev).bfloat16()
        gamma = torch.randn(C, device=dev) * 0.3
        dout = torch.randn(N, C, H, W, device=dev)
        d16 = torch.randn(N, C, H, W, device=dev).bfloat16()
        for with_scale in (False, True):
            scale = (torch.rand(N, device=dev) > 0.3).float() / 0.7 if with_scale else None
            sd = scale.double().view(N, 1, 1, 1) if with_scale else 1.0
            for sc_dtype in (torch.float32, torch.bfloat16):
                sc = torch.randn(N, C, H, W, device=dev).to(sc_dtype)
                ref = sc.double() + (gamma.double() * z.double()).permute(0, 3, 1, 2) * sd
                op = "sr_fwd/f32" if sc_dtype == torch.float32 else "sr_fwd/bf16"

                def sr_fwd():
                    out, out16 = _sr_fwd_ld(L, sc, z, gamma, scale, None, sc_dtype == torch.float32)     # the bf16 copy as a training step asks for it
                    assert out16 is None or torch.equal(out16, out.bfloat16()), "the bf16 copy is not the rounded output"
                    return err(out, ref, 1e-6, "out")
                doc.check("%s/%s%s" % (tag, op, "/scaled" if with_scale else ""), fam_of(case, op), sr_fwd)
            for second in (None, d16):
                d = dout.double() + (second.double() if second is not None else 0.0)
                ds = d * sd
                dz_ref = (ds * gamma.double().view(1, C, 1, 1)).permute(0, 2, 3, 1)

                def sr_bwd():
                    dsum, dz, dg, dzc = _sr_bwd_ld(L, dout, second, z, gamma, scale, None)
                    e = max(err(dz, dz_ref, 2.0 ** -8 * 1.01, "dz"), err(dg, (ds.permute(0, 2, 3, 1) * z.double()).sum((0, 1, 2)), 1e-4, "dgamma"),
                            err(dzc, dz_ref.sum((0, 1, 2)), 1e-4, "column sums of dz"))
                    return e if second is None else max(e, err(dsum, d, 1e-6, "dshortcut"))
                doc.check("%s/sr_bwd%s%s" % (tag, "/scaled" if with_scale else "", "/two gradients" if second is not None else ""), fam_of(case, "sr_bwd"), sr_bwd)
    torch.cuda.synchronize()


def _ln_cf_child(doc, name, dev):
    """test_ln_channels_first_matches_explicit_ops (models/SLaK.py:257-260 in fp64) with the one-pass backward kernel off."""
    import torch
    from slak_amd import _lib, block_ops
    from tail_calls import _close
    L = _lib.lib()
    obs = doc.d["observable"]

    def err(a, b, rel, what):
        _close(a, b, rel, what)
        return (a.double() - b.double()).abs().max().item() / max(1e-6, b.double().abs().max().item())

    for case in SWITCHES[name]["cases"]:
        N, C, H, W = case
        obs[tail_key(case)] = {"backward_pair_supported": int(L.slak_ln_channels_first_backward_pair_supported(_lib.SLAK_F32, _lib.SLAK_BF16, N, C, H * W))}
        for in_dtype in (torch.float32, torch.bfloat16):
            torch.manual_seed(C)
            x = (torch.randn(N, C, H, W, device=dev) * 1.5 + 0.2).to(in_dtype).requires_grad_(True)
            w = (torch.randn(C, device=dev) * 0.5 + 1).requires_grad_(True); b = (torch.randn(C, device=dev) * 0.1).requires_grad_(True)
            g = torch.randn(N, C, H, W, device=dev)
            xr = x.detach().double().requires_grad_(True); wr = w.detach().double().requires_grad_(True); br = b.detach().double().requires_grad_(True)
            u = xr.mean(1, keepdim=True); s = (xr - u).pow(2).mean(1, keepdim=True)
            yr = wr[:, None, None] * ((xr - u) / torch.sqrt(s + 1e-6)) + br[:, None, None]
            yr.backward(g.double())

            def run():
                y = block_ops.ln_channels_first(x, w, b, 1e-6, torch.float32)
                y.backward(g)
                return max(err(y.detach(), yr.detach(), 2e-6, "y"), err(x.grad, xr.grad, 2.0 ** -8 * 1.05 if in_dtype == torch.bfloat16 else 2e-5, "dx"),
                           err(w.grad, wr.grad, 1e-4, "dw"), err(b.grad, br.grad, 1e-4, "db"))
            doc.check("%s/ln_channels_first/%s" % (tail_key(case), "bf16" if in_dtype == torch.bfloat16 else "f32"), "ln_cf_fwd + ln_cf_bwd (two-pass)", run)
    torch.cuda.synchronize()


def _pointwise_child(doc, name, dev):
    import torch
    import torch.nn.functional as F
    from slak_amd import _lib, block_ops
    from tail_calls import _close
    L = _lib.lib()
    obs = doc.d["observable"]
    st = torch.cuda.current_stream(dev).cuda_stream
    bf = torch.bfloat16
    nan = float("nan")

    def err(a, b, rel, what):
        _close(a, b, rel, what)
        return (a.double() - b.double()).abs().max().item() / max(1e-6, b.double().abs().max().item())

    def within(got, ref, bound, what):
        e = (got.double() - ref).abs()
        assert (e <= bound).all(), "%s: exceeds its bound by %.3e" % (what, float((e - bound).max()))
        return e.max().item()

    def product_bound(ref):                                 # test_linear_nt_matches_fp64_product / test_gemm_with_gelu_epilogue_...: half a bf16 ulp + fp32 accumulation
        return 2.0 ** -8 * ref.abs() + 1e-5 * max(1.0, ref.abs().max().item())

    def gelu_of_rounded(y, a):                              # the same two tests: GELU of the ROUNDED pre-activation, at most one bf16 ulp, > 98 % identical
        want = F.gelu(y.float()).to(bf)
        d = (a.float() - want.float()).abs()
        assert (d <= 2.0 ** -7 * want.float().abs() + 1e-6).all(), d.max().item()
        assert (d == 0).float().mean().item() > 0.98
        return d.max().item()

    def dgelu_ref(dz, w2t, y1):                             # test_gemm_with_gelu_backward_epilogue_on_random_operands_vs_fp64
        dact = dz.double() @ w2t.double().t()
        yy = y1.double()
        gp = 0.5 * (1 + torch.erf(yy / math.sqrt(2))) + yy * torch.exp(-0.5 * yy * yy) / math.sqrt(2 * math.pi)
        want = dact * gp
        return want, 2.0 ** -7 * want.abs() + 2.0 ** -8 * dact.abs() + 1e-6

    for case in SWITCHES[name]["cases"]:
        M, C = case["M"], case["C"]
        C4 = 4 * C
        tag = "m%d_c%d" % (M, C)
        rungs = mlp_rungs(L, _lib, M, C)
        obs[tag] = {"plan": rungs, "expect": case["expect"], "as_expected": all(rungs[k] == v for k, v in case["expect"].items())}
        # test_mlp_splitk_matches_torch: pwconv2(gelu(pwconv1(t))) and its five gradients against fp64 on the same bf16 operands
        torch.manual_seed(M)
        t = torch.randn(M, C, device=dev).bfloat16().requires_grad_(True)
        w1 = (torch.randn(C4, C, device=dev) * 0.05).requires_grad_(True); b1 = (torch.randn(C4, device=dev) * 0.05).requires_grad_(True)
        w2 = (torch.randn(C, C4, device=dev) * 0.05).requires_grad_(True); b2 = (torch.randn(C, device=dev) * 0.05).requires_grad_(True)
        dz = torch.randn(M, C, device=dev).bfloat16()
        td = t.detach().double().requires_grad_(True)
        ps = [p.detach().bfloat16().double().requires_grad_(True) for p in (w1, b1, w2, b2)]
        zr = F.linear(F.gelu(F.linear(td, ps[0], ps[1])), ps[2], ps[3])
        zr.backward(dz.double())

        def mlp():
            z = block_ops.mlp_splitk(t, w1, b1, w2, b2)
            z.backward(dz)
            e = [err(z.detach(), zr.detach(), 1.5e-2, "z"), err(t.grad, td.grad, 2e-2, "dt")]
            e += [err(got, ref, 2e-2, n) for got, ref, n in ((w1.grad, ps[0].grad, "dw1"), (b1.grad, ps[1].grad, "db1"), (w2.grad, ps[2].grad, "dw2"), (b2.grad, ps[3].grad, "db2"))]
            return max(e)
        doc.check(tag + "/mlp_splitk", " ".join("%s=%s" % kv for kv in rungs.items()), mlp)
        # the direct entry points on the same shape: each runs where its own query says yes, and is recorded as declined where it says 0
        x = t.detach()
        w1b, b1b, w2b, b2b = (p.detach().to(bf).contiguous() for p in (w1, b1, w2, b2))
        w2t, w1t = w2b.t().contiguous(), w1b.t().contiguous()
        a = (torch.randn(M, C4, device=dev) * 0.5).to(bf)
        y1 = torch.randn(M, C4, device=dev).to(bf)

        if L.slak_linear_nt_supported(M, C4, C, 1):
            def nt_gelu():
                y, ga = block_ops.linear_nt(x, w1b, b1b, gelu=True)
                return max(within(y, x.double() @ w1b.double().t() + b1b.double(), product_bound(x.double() @ w1b.double().t() + b1b.double()), "y1"), gelu_of_rounded(y, ga))
            doc.check(tag + "/linear_nt(gelu)", "linear_nt", nt_gelu)
        else:
            doc.declined(tag + "/linear_nt(gelu)")
        if L.slak_linear_nt_supported(M, C, C4, 0):
            def nt():
                ref = a.double() @ w2b.double().t() + b2b.double()
                return within(block_ops.linear_nt(a, w2b, b2b), ref, product_bound(ref), "z")
            doc.check(tag + "/linear_nt", "linear_nt", nt)
        else:
            doc.declined(tag + "/linear_nt")
        if L.slak_linear_mlp_fwd_supported(M, C, C4):
            def mlp_fwd():                                   # test_linear_mlp_fwd_is_pwconv1_gelu_pwconv2: z against the fp64 product of the STORED a
                yo = torch.full((M, C4), nan, device=dev, dtype=bf); ao = torch.full_like(yo, nan); zo = torch.full((M, C), nan, device=dev, dtype=bf)
                _lib.check(L.slak_linear_mlp_fwd(x.data_ptr(), w1b.data_ptr(), b1b.data_ptr(), w2b.data_ptr(), b2b.data_ptr(), yo.data_ptr(), ao.data_ptr(), zo.data_ptr(),
                                                 M, C, C4, st), "slak_linear_mlp_fwd")
                r1 = x.double() @ w1b.double().t() + b1b.double()
                ref = ao.double() @ w2b.double().t() + b2b.double()
                return max(within(yo, r1, product_bound(r1), "y1"), gelu_of_rounded(yo, ao), within(zo, ref, ref.abs() * 2.0 ** -8 * 1.01 + 1e-4, "z"))
            doc.check(tag + "/linear_mlp_fwd", "linear_mlp_fwd", mlp_fwd)
        else:
            doc.declined(tag + "/linear_mlp_fwd")
        want, bound = dgelu_ref(dz, w2t, y1)
        for fused_dt in (False, True):
            what = "linear_nt_gelu_bwd_dt" if fused_dt else "linear_nt_gelu_bwd"
            if not (L.slak_linear_nt_gelu_bwd_dt_supported if fused_dt else L.slak_linear_nt_gelu_bwd_supported)(M, C4, C):
                doc.declined(tag + "/" + what)
                continue

            def gelu_bwd(fused_dt=fused_dt, what=what):
                nb = int(L.slak_linear_nt_gelu_bwd_workspace_bytes(M, C4, C))
                ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
                dy1 = torch.full((M, C4), nan, device=dev, dtype=bf); db = torch.full((C4,), nan, device=dev); dt = torch.full((M, C), nan, device=dev, dtype=bf)
                if fused_dt:
                    w1p = w1t.view(3, 32, 6, 4, 2, 8).permute(2, 3, 0, 4, 1, 5).contiguous()
                    _lib.check(L.slak_linear_nt_gelu_bwd_dt(dz.data_ptr(), w2t.data_ptr(), y1.data_ptr(), w1p.data_ptr(), dy1.data_ptr(), dt.data_ptr(), db.data_ptr(),
                                                            M, C4, C, ws.data_ptr(), nb, st), what)
                else:
                    _lib.check(L.slak_linear_nt_gelu_bwd(dz.data_ptr(), w2t.data_ptr(), y1.data_ptr(), dy1.data_ptr(), db.data_ptr(), M, C4, C, ws.data_ptr(), nb, st), what)
                e = within(dy1, want, bound, "dy1")
                col = dy1.double().sum(0)                   # test_linear_nt_gelu_bwd_is_the_gemm_followed_by_the_gelu_backward: column sums of the stored dy1
                assert (db.double() - col).abs().max().item() <= 1e-5 * max(1.0, col.abs().max().item()) * max(1.0, M ** 0.5 / 30), "db1"
                if fused_dt:                                # test_linear_nt_gelu_bwd_dt_adds_the_next_product
                    wdt = dy1.double() @ w1t.double().t()
                    assert (dt.double() - wdt).abs().max().item() <= 2.0 ** -8 * 1.05 * wdt.abs().max().item(), "dt"
                return e
            doc.check(tag + "/" + what, what, gelu_bwd)
        for epi, ename in ((1, "gelu"), (2, "dgelu")):
            if not L.slak_linear_gemm_supported(M, C4, C, epi):
                doc.declined(tag + "/linear_gemm(%s)" % ename)
                continue

            def gemm(epi=epi):
                nb = int(L.slak_linear_gemm_workspace_bytes(M, C4, C, epi))
                ws = torch.empty(max(nb, 16), device=dev, dtype=torch.uint8)
                out = torch.full((M, C4), nan, device=dev, dtype=bf)
                out2 = torch.full((M, C4), nan, device=dev, dtype=bf) if epi == 1 else None
                db = torch.full((C4,), nan, device=dev) if epi == 2 else None
                _lib.check(L.slak_linear_gemm((x if epi == 1 else dz).data_ptr(), (w1b if epi == 1 else w2t).data_ptr(), b1b.data_ptr() if epi == 1 else None, out.data_ptr(),
                                              out2.data_ptr() if epi == 1 else None, y1.data_ptr() if epi == 2 else None, db.data_ptr() if epi == 2 else None,
                                              M, C4, C, epi, ws.data_ptr() if nb else None, nb, st), "slak_linear_gemm")
                if epi == 1:
                    ref = x.double() @ w1b.double().t() + b1b.double()
                    return max(within(out, ref, product_bound(ref), "y1"), gelu_of_rounded(out, out2))
                e = within(out, want, bound, "dy1")
                assert ((db.double() - out.double().sum(0)).abs() <= 1e-5 * out.double().abs().sum(0) + 1e-6).all(), "db1"
                return e
            doc.check(tag + "/linear_gemm(%s)" % ename, "linear_gemm", gemm)
        for n1, n2 in [(C4, C), (C, C4)] + case.get("wgrad", []):
            what = "%s/linear_wgrad(%d,%d)" % (tag, n1, n2)
            if not (M >= 1 and L.slak_linear_wgrad_supported(M, n1, n2)):
                doc.declined(what)
                continue

            def wgrad(n1=n1, n2=n2):                        # test_linear_wgrad_matches_fp32
                dy = torch.randn(M, n1, device=dev).to(bf)
                xx = (torch.randn(M, n2, device=dev) + 0.25).to(bf)
                d = block_ops.linear_wgrad(dy, xx)
                assert d is not None, "declined after slak_linear_wgrad_supported said yes"
                ref = dy.double().t() @ xx.double()
                e = (d.double() - ref).abs().max().item()
                assert e <= 1e-5 * ref.abs().max().item() + 1e-6, e
                return e
            doc.check(what, "linear_wgrad", wgrad)
    torch.cuda.synchronize()


def main(name):
    sw = SWITCHES[name]
    assert os.environ.get(name) == sw["flip"], "%s must be %s in this process's environment" % (name, sw["flip"])
    for p in (ROOT, TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    t0 = time.time()
    import torch
    dev = torch.device("cuda:0")
    doc = _Doc(name)
    {"conv": _conv_child, "tail": _tail_child, "ln_cf": _ln_cf_child, "pointwise": _pointwise_child}[sw["group"]](doc, name, dev)
    doc.d["seconds"] = round(time.time() - t0, 2)
    print(json.dumps(doc.d))


if __name__ == "__main__":
    main(sys.argv[1])
