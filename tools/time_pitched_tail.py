"""Kernel times of the pitched block-tail entry points (slak_*_ld) at the four stage shapes of SLaK at width_factor 1.3, batch 128 --
C = 124 @ 56x56, 249 @ 28x28, 499 @ 14x14, 998 @ 7x7 with rows of ldc = 128 / 256 / 512 / 1024 -- next to the plain entry points on a tensor
with C = ldc channels of the same N and P (the sibling moves at least as many bytes).

    python tools/time_pitched_tail.py [--batch 128] [--reps 20] [--rounds 7]

Device events around `reps` back-to-back launches, `rounds` rounds per entry point, pitched and sibling rounds alternating; one JSON line
per (shape, op): the median round in us per launch and the spread (min, max) of both, and beside each time the kernel family that
slak_block_tail_family names for the call (tile / reg / chan / chan1).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

SHAPES = [(124, 56, 128), (249, 28, 256), (499, 14, 512), (998, 7, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_pitched_tail.py needs an MI355X")
    from slak_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    N = a.batch
    fam_op = {"ln_fwd": _lib.TAIL_LN_FWD, "ln_bwd": _lib.TAIL_LN_BWD, "sr_fwd": _lib.TAIL_SR_FWD, "sr_bwd": _lib.TAIL_SR_BWD}

    def family(name, Cx, P, pitch):
        return _lib.TAIL_FAMILY_NAMES[L.slak_block_tail_family(fam_op[name], _lib.SLAK_F32, N, Cx, P, pitch)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.reps

    for C, HW, ldc in SHAPES:
        P = HW * HW
        torch.manual_seed(C)

        def operands(Cx, pitch):
            o = {"x": torch.randn(N, Cx, P, device=dev).bfloat16(), "w": torch.randn(Cx, device=dev), "b": torch.randn(Cx, device=dev),
                 "y": torch.zeros(N, P, pitch, device=dev, dtype=torch.bfloat16), "mean": torch.empty(N, P, device=dev), "rstd": torch.empty(N, P, device=dev),
                 "g": torch.randn(N, P, pitch, device=dev).bfloat16(), "dx": torch.empty(N, Cx, P, device=dev, dtype=torch.bfloat16),
                 "dw": torch.empty(Cx, device=dev), "db": torch.empty(Cx, device=dev), "sc": torch.randn(N, Cx, P, device=dev),
                 "out": torch.empty(N, Cx, P, device=dev), "out16": torch.empty(N, Cx, P, device=dev, dtype=torch.bfloat16),
                 "dout": torch.randn(N, Cx, P, device=dev), "d16": torch.randn(N, Cx, P, device=dev).bfloat16(), "dsum": torch.empty(N, Cx, P, device=dev),
                 "dz": torch.empty(N, P, pitch, device=dev, dtype=torch.bfloat16)}
            nb = int(L.slak_block_tail_workspace_bytes(N, pitch, P))
            o["ws"], o["nb"] = torch.empty(nb, dtype=torch.uint8, device=dev), nb
            return o

        def ops(o, Cx, pitch, ld):
            tail = (pitch,) if ld else ()
            sfx = "_ld" if ld else ""
            p = {k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in o.items()}
            return {
                "ln_fwd": lambda: _lib.check(getattr(L, "slak_ln_nchw_to_nhwc_forward" + sfx)(p["x"], p["w"], p["b"], p["y"], p["mean"], p["rstd"], N, Cx, P, 1e-6, st, *tail)),
                "ln_bwd": lambda: _lib.check(getattr(L, "slak_ln_nchw_to_nhwc_backward" + sfx)(p["g"], p["x"], p["w"], p["mean"], p["rstd"], p["dx"], p["dw"], p["db"], N, Cx, P,
                                                                                                 p["ws"], p["nb"], st, *tail)),
                "sr_fwd": lambda: _lib.check(getattr(L, "slak_scale_residual_forward" + sfx)(p["sc"], _lib.SLAK_F32, p["g"], p["w"], None, p["out"], p["out16"], N, Cx, P, st, *tail)),
                "sr_bwd": lambda: _lib.check(getattr(L, "slak_scale_residual_backward" + sfx)(p["dout"], p["d16"], p["dsum"], p["g"], p["w"], None, p["dz"], p["dw"], p["db"],
                                                                                                N, Cx, P, p["ws"], p["nb"], st, *tail)),
            }

        po, so = operands(C, ldc), operands(ldc, ldc)
        pitched, sibling = ops(po, C, ldc, True), ops(so, ldc, ldc, False)
        for name in ("ln_fwd", "ln_bwd", "sr_fwd", "sr_bwd"):
            for _ in range(3):
                pitched[name](); sibling[name]()
            torch.cuda.synchronize()
            tp, ts = [], []
            for _ in range(a.rounds):
                tp.append(timed(pitched[name])); ts.append(timed(sibling[name]))
            print(json.dumps({"op": name, "N": N, "C": C, "P": P, "ldc": ldc,
                              "pitched_family": family(name, C, P, ldc), "sibling_family": family(name, ldc, P, ldc),
                              "pitched_us": round(statistics.median(tp), 2), "pitched_min_max_us": [round(min(tp), 2), round(max(tp), 2)],
                              "sibling_C_eq_ldc_us": round(statistics.median(ts), 2), "sibling_min_max_us": [round(min(ts), 2), round(max(ts), 2)]}), flush=True)
        del po, so, pitched, sibling
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
