"""The tail of the training step -- global average pool, final LayerNorm, head Linear, criterion, forward and backward -- on the fused ops
(block_ops.pool_ln, slak_amd.loss) next to the PyTorch ops it replaces, at the shapes of SLaK-T's last stage (width 1.0 and 1.3):
N = 128, P = 7 x 7, K = 1000, C = 768 / 998, bf16 autocast.

    python tools/time_head_loss.py [--batch 128] [--reps 20] [--rounds 7]

Per (C, criterion): the device launches of one forward + backward (counted by torch.profiler: kernels and memory operations), and device
events around `reps` back-to-back forward + backward passes, `rounds` rounds per path, fused and torch rounds alternating; the median round in
us per pass and its spread.  The passes are issued from Python, so a time includes whatever the device waits for the host between launches:
that wait is what the fused path removes.  Prints ONE JSON line.
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
import torch.nn as nn
import torch.nn.functional as F


def count_launches(fn):
    """device-side events (kernels, copies, fills) of one call of fn; None where the profiler records no device activity"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_head_loss.py needs an MI355X")
    import slak_amd
    from slak_amd import block_ops, loss as LS
    dev = torch.device("cuda", 0)
    N, P, K = a.batch, 49, 1000
    results = []
    for C in (768, 998):
        torch.manual_seed(C)
        x = torch.randn(N, C, 7, 7, device=dev, requires_grad=True)
        norm = nn.LayerNorm(C, eps=1e-6).to(dev)
        head = nn.Linear(C, K).to(dev)
        labels = torch.randint(0, K, (N,), device=dev)
        soft = torch.full((N, K), 0.1 / K, device=dev)                       # mixup's shape, built once
        soft[torch.arange(N, device=dev), labels] += 0.9 * 0.7
        soft[torch.arange(N, device=dev), labels.flip(0)] += 0.9 * 0.3
        params = [x] + list(norm.parameters()) + list(head.parameters())

        def soft_torch(z, t):                                                # timm1/loss/cross_entropy.py:34-36
            return torch.sum(-t * F.log_softmax(z, dim=-1), dim=-1).mean()

        cases = {"label_smoothing": (slak_amd.LabelSmoothingCrossEntropy(0.1), nn.CrossEntropyLoss(label_smoothing=0.1), labels),
                 "soft_target": (slak_amd.SoftTargetCrossEntropy(), soft_torch, soft)}
        for cname, (crit_fused, crit_torch, target) in cases.items():
            def fused():
                for p in params:
                    p.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    loss = crit_fused(head(block_ops.pool_ln(x, norm.weight, norm.bias, norm.eps)), target)
                loss.backward()
                return loss

            def plain():
                for p in params:
                    p.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    loss = crit_torch(head(norm(x.mean([-2, -1]))), target)
                loss.backward()
                return loss

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                return 1e3 * e0.elapsed_time(e1) / a.reps

            for _ in range(5):
                lf = fused(); lp = plain()
            torch.cuda.synchronize()
            h0, f0 = block_ops.head_hits, LS.fused_hits
            tf, tp = [], []
            for _ in range(a.rounds):
                tf.append(timed(fused)); tp.append(timed(plain))
            hits = (block_ops.head_hits - h0, LS.fused_hits - f0)
            assert hits == (a.rounds * a.reps, a.rounds * a.reps), hits      # the fused path really ran on the kernels
            results.append({"C": C, "criterion": cname, "N": N, "P": P, "K": K,
                            "fused_launches": count_launches(fused), "torch_launches": count_launches(plain),
                            "fused_us": round(statistics.median(tf), 2), "fused_min_max_us": [round(min(tf), 2), round(max(tf), 2)],
                            "torch_us": round(statistics.median(tp), 2), "torch_min_max_us": [round(min(tp), 2), round(max(tp), 2)],
                            "loss_fused": float(lf), "loss_torch": float(lp)})
    print(json.dumps({"tool": "time_head_loss", "reps": a.reps, "rounds": a.rounds, "gpu": torch.cuda.get_device_name(0), "cases": results}), flush=True)


if __name__ == "__main__":
    main()
