"""What happens to the gradients between backward() and the optimizer step, three ways, on SLaK-T 51x51, 224 px, batch 128, bf16 autocast with the
switches bench.py turns on:

    python tools/time_grad_norm.py [--clip-grad V] [--batch 128] [--reps 10] [--rounds 7] [--out FILE.jsonl]

  (a) reference : utils.NativeScalerWithGradNormCount.__call__ (utils.py:384-404) as written, on MaskedAdamW: GradScaler.scale(loss).backward(),
                  unscale_, get_grad_norm_ (one torch.norm per parameter) or clip_grad_norm_ with --clip-grad, scaler.step(optimizer) (its .item()
                  synchronises the host), scaler.update()
  (b) fused     : slak_amd.scaler.NativeScalerWithGradNormCount -> MaskedAdamW.step_with_grad_norm
  (c) plain     : loss.backward(); optimizer.step() -- no norm, no clipping, no loss scale: what bench.py times

Per path: the device launches between the end of backward and the end of the update (torch.profiler: kernels and memory operations), and the
step time: `reps` whole training steps between two synchronisations, `rounds` rounds per path, the three paths alternating; the median round in
ms per step and its min / max.  (a) and (b) carry the same GradScaler (2^16; bf16 gradients do not overflow, so no step is skipped).
Prints ONE JSON line per path, and appends them to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.nn as nn


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
    ap.add_argument("--clip-grad", type=float, default=None)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--prime", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_grad_norm.py needs an MI355X (no CPU fallback for the hot path)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.backends.cudnn.benchmark = True
    import slak_amd.slak_model as M
    from slak_amd import block_ops
    from slak_amd.optim_factory import MaskedAdamW
    from slak_amd.scaler import NativeScalerWithGradNormCount, get_grad_norm_
    M.Block.fused_tail = True
    M.ReparamLargeKernelConv.fused_bn = True
    M.LayerNorm.fused_cf = True
    M.SLaK.fused_stem = True
    M.SLaK.fused_downsample = True
    M.ReparamLargeKernelConv.fused_tri = True
    M.Block.fused_block = True
    block_ops.cache_lowp_weights = True
    M.use_sync_bn = True
    torch.manual_seed(0)
    model = M.create_model("SLaK_tiny", kernel_size=[51, 49, 47, 13, 5], Decom=True, bn=True, drop_path_rate=0.1, lowp_dwconv=True).to(device)
    decay, no_decay = [], []
    for n, p in model.named_parameters():
        (no_decay if (p.dim() == 1 or n.endswith(".bias")) else decay).append(p)
    opt = MaskedAdamW([dict(params=decay, weight_decay=0.05), dict(params=no_decay, weight_decay=0.0)], lr=4e-3)
    params = decay + no_decay
    criterion = nn.CrossEntropyLoss(label_smoothing=0.1)
    g = torch.Generator(device=device).manual_seed(1234)
    samples = torch.randn(a.batch, 3, a.res, a.res, device=device, generator=g)
    targets = torch.randint(0, 1000, (a.batch,), device=device, generator=g)
    ref_scaler = torch.amp.GradScaler("cuda")
    fused_scaler = NativeScalerWithGradNormCount()
    norms = {}

    def forward():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return criterion(model(samples), targets)

    # each path as (backward, update): the launches of `update` are the ones counted
    def ref_backward(loss):
        ref_scaler.scale(loss).backward()

    def ref_update():                                                # utils.py:392-401
        ref_scaler.unscale_(opt)
        if a.clip_grad is not None:
            norms["reference"] = torch.nn.utils.clip_grad_norm_(params, a.clip_grad)
        else:
            norms["reference"] = get_grad_norm_(params)
        ref_scaler.step(opt)
        ref_scaler.update()

    def fused_backward(loss):
        fused_scaler._scaler.scale(loss).backward()

    def fused_update():
        norms["fused"] = fused_scaler._fused_update(opt, a.clip_grad)

    def plain_backward(loss):
        loss.backward()

    paths = {"reference": (ref_backward, ref_update), "fused": (fused_backward, fused_update), "plain": (plain_backward, opt.step)}

    def step(name):
        backward, update = paths[name]
        loss = forward()
        backward(loss)
        update()
        opt.zero_grad(set_to_none=True)
        return loss

    def timed(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            step(name)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.reps

    model.train()
    for _ in range(a.prime):
        for name in paths:
            loss = step(name)
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(a.rounds):
        for name in paths:
            times[name].append(timed(name))
    launches = {}
    for name, (backward, update) in paths.items():
        backward(forward())
        launches[name] = count_launches(update)
        opt.zero_grad(set_to_none=True)
    lines = []
    for name in paths:
        t = times[name]
        lines.append({"tool": "time_grad_norm", "path": name, "clip_grad": a.clip_grad, "ms_per_step": round(statistics.median(t), 4),
                      "min_max_ms": [round(min(t), 4), round(max(t), 4)], "spread_ms": round(max(t) - min(t), 4),
                      "launches_after_backward": launches[name], "grad_norm": float(norms[name]) if name in norms else None,
                      "workload": "SLaK-T 51x51, bs=%d, %dx%d, bf16, MaskedAdamW" % (a.batch, a.res, a.res),
                      "reps": a.reps, "rounds": a.rounds, "final_loss": float(loss.detach()), "gpu": torch.cuda.get_device_name(0)})
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
