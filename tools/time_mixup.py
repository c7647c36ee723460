"""Time of one ``Mixup.__call__`` on the HIP kernels against the reference's op sequence as torch ops (slak_amd.mixup's formula path: the yardstick is
the reference's sequence, not the code under test), at the recipes' shape: N = 128, 3 x 224 x 224 float32, K = 1000.

    python tools/time_mixup.py [--out profiles/mixup_kernels.jsonl] [--calls 20] [--rounds 7]
    python tools/time_mixup.py --launches            # a separate run: device launches per call, counted by the profiler

Modes: batch mixup, batch CutMix, 'elem' with the recipes' setting.  Device events around ``--calls`` calls, ``--rounds`` rounds per path, kernel and
formula rounds ALTERNATING in one process, both from the same seed per round (the same parameters); median and min-max of the rounds.  One JSON line per
mode.  ``image_pass_*``: the image kernel alone (batch mixup record, back-to-back launches) and its share of 8 TB/s on 2 N C H W 4 bytes (reported,
not gated).  Needs an MI355X: there is nothing to time without one.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

N, C, H, W, K = 128, 3, 224, 224, 1000
MODES = {
    "batch_mixup": dict(mixup_alpha=0.8, cutmix_alpha=0.0, mode="batch"),
    "batch_cutmix": dict(mixup_alpha=0.0, cutmix_alpha=1.0, mode="batch"),
    "elem_recipe": dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem"),
}


@contextlib.contextmanager
def formula_only(mixup):
    saved = mixup._images_ok, mixup._labels_ok
    mixup._images_ok, mixup._labels_ok = (lambda x: False), (lambda *a: False)
    try:
        yield
    finally:
        mixup._images_ok, mixup._labels_ok = saved


def events_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixup_kernels.jsonl"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", action="store_true", help="count device launches per call with the profiler instead of timing")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_mixup.py needs an MI355X")
    from slak_amd import mixup
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)
    x = torch.randn(N, C, H, W, device=dev, generator=g)
    y = torch.randint(0, K, (N,), device=dev, generator=g)
    lines = []
    for name, cfg in MODES.items():
        fn = mixup.Mixup(label_smoothing=0.1, num_classes=K, **cfg)
        call = lambda: fn(x, y)
        if a.launches:
            from torch.profiler import ProfilerActivity, profile
            counts = {}
            for path in ("kernels", "formula"):
                with (formula_only(mixup) if path == "formula" else contextlib.nullcontext()):
                    np.random.seed(0)
                    call()
                    torch.cuda.synchronize()
                    np.random.seed(1)
                    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                        call()
                        torch.cuda.synchronize()
                dev_events = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
                counts[path] = {"device_launches": len(dev_events), "copies": sum("memcpy" in e.name.lower() for e in dev_events)}
            lines.append({"mode": name, "what": "device launches of one call (profiler, separate run)", **counts})
            continue
        for path in ("kernels", "formula"):                      # warm both paths up
            with (formula_only(mixup) if path == "formula" else contextlib.nullcontext()):
                np.random.seed(0)
                for _ in range(3):
                    call()
        torch.cuda.synchronize()
        t = {"kernels": [], "formula": []}
        hits = mixup.fused_hits
        for r in range(a.rounds):
            for path in ("kernels", "formula"):
                with (formula_only(mixup) if path == "formula" else contextlib.nullcontext()):
                    np.random.seed(100 + r)
                    torch.cuda.synchronize()
                    t[path].append(events_ms(call, a.calls))
        assert mixup.fused_hits - hits == a.rounds * a.calls
        line = {"mode": name, "shape": [N, C, H, W], "classes": K, "calls_per_round": a.calls, "rounds": a.rounds,
                "kernels": spread(t["kernels"]), "formula": spread(t["formula"]),
                "formula_over_kernels": round(statistics.median(t["formula"]) / statistics.median(t["kernels"]), 2),
                "gpu": torch.cuda.get_device_name(0)}
        if name == "batch_mixup":
            staged = mixup._Staged(mixup.Record(mixup.MIX, 0.7, 0.3, 0, 0, 0, 0), None, dev)
            one = lambda: mixup._mix_launch(x, staged)
            one()
            torch.cuda.synchronize()
            v = [events_ms(one, a.calls) for _ in range(a.rounds)]
            nbytes = 2 * N * C * H * W * 4
            line["image_pass"] = dict(spread(v), bytes=nbytes, share_of_8TBps=round(nbytes / (statistics.median(v) * 1e-3) / 8e12, 3))
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.launches else "w") as f:              # the launch counts go behind the timings of the earlier run
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
