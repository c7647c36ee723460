"""Step time of SLaK-T / -S / -B at a width factor (default 1.3: the width of every README recipe, C = 124 / 249 / 499 / 998 for SLaK-T and -S),
with bench.py's protocol:

    python tools/time_width.py [--model tiny|small|base] [--width 1.3] [--batch 128] [--res 224] [--steps 20] [--warmup 5] [--prime 15]

224 px, bf16 autocast, batch 128, MaskedAdamW, every fused path bench.py turns on; prime + warm-up steps, then K steps between two
synchronisations.  Prints ONE JSON line: ms_per_step, host_enqueue_ms_per_step (three steps enqueued on a drained queue, the quietest of three
rounds), pitched_block_hits (block forwards that ran on pitched NHWC tensors: 0 on a tree without them, and at width 1.0) and
pitched_runner_hits (those of them that the C++ block runner issued).  SLaK-B at width 1.3 (C = 166 / 332 / 665 / 1331) is outside the fused
block path in stage 4 (C > 1024): its blocks there run the PyTorch ops.
SLAK_PAD_EVEN=1 also pads the even widths 124 / 998 (block_ops.pad_even_widths).  bench.py itself has no width switch.
--fused-head turns SLaK.fused_head on; --criterion label_smoothing | soft_target runs the criterion of slak_amd.loss (its HIP kernel) instead of
torch's nn.CrossEntropyLoss(label_smoothing=0.1); head_hits_per_step / fused_hits_per_step count the calls the two kernels served.
--mixup (with --criterion soft_target) runs slak_amd.mixup.Mixup with the recipes' setting (mixup 0.8, cutmix 1.0, smoothing 0.1, 'batch' mode) on the
batch and the hard labels in every step, as engine.py:49-50 does, and adds "mixup" / "mixup_hits_per_step" to the line; without the flag nothing changes.
--clip-grad V takes the step through MaskedAdamW.step_with_grad_norm(clip_grad=V) (gradient norm, clipping and the step on 2 * plans + 1 launches:
DESIGN 11); --scaler drives backward and the step through slak_amd.scaler.NativeScalerWithGradNormCount(enabled=False) (bf16 needs no loss scaling),
with --clip-grad's value if given.  Either adds "clip_grad" / "scaler" / "grad_norm" to the line; without them the step is opt.step() as before.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.nn as nn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("tiny", "small", "base"), default="tiny")
    ap.add_argument("--width", type=float, default=1.3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prime", type=int, default=15)
    ap.add_argument("--fused-head", action="store_true", help="SLaK.fused_head: pool + final LayerNorm as one launch (block_ops.pool_ln)")
    ap.add_argument("--criterion", choices=("label_smoothing", "soft_target"), default=None,
                    help="the criterion of slak_amd.loss on its HIP kernel (default: torch's nn.CrossEntropyLoss(label_smoothing=0.1))")
    ap.add_argument("--mixup", action="store_true", help="slak_amd.mixup.Mixup on every batch (needs --criterion soft_target)")
    ap.add_argument("--clip-grad", type=float, default=None, help="step through MaskedAdamW.step_with_grad_norm(clip_grad=V)")
    ap.add_argument("--scaler", action="store_true", help="backward + step through slak_amd.scaler.NativeScalerWithGradNormCount(enabled=False)")
    a = ap.parse_args()
    if a.mixup and a.criterion != "soft_target":
        ap.error("--mixup needs --criterion soft_target (main.py:397-399)")
    if not torch.cuda.is_available():
        sys.exit("tools/time_width.py needs an MI355X (no CPU fallback for the hot path)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.backends.cudnn.benchmark = True
    import slak_amd.slak_model as M
    from slak_amd import block_ops
    from slak_amd.optim_factory import MaskedAdamW
    M.Block.fused_tail = True
    M.ReparamLargeKernelConv.fused_bn = True
    M.LayerNorm.fused_cf = True
    M.SLaK.fused_stem = True
    M.SLaK.fused_downsample = True
    M.ReparamLargeKernelConv.fused_tri = True
    M.Block.fused_block = True
    block_ops.cache_lowp_weights = True
    M.use_sync_bn = True
    if a.fused_head:
        M.SLaK.fused_head = True
    torch.manual_seed(0)
    model = M.create_model("SLaK_" + a.model, kernel_size=[51, 49, 47, 13, 5], Decom=True, bn=True, drop_path_rate=0.1, lowp_dwconv=True,
                           width_factor=a.width).to(device)
    decay, no_decay = [], []
    for n, p in model.named_parameters():
        (no_decay if (p.dim() == 1 or n.endswith(".bias")) else decay).append(p)
    opt = MaskedAdamW([dict(params=decay, weight_decay=0.05), dict(params=no_decay, weight_decay=0.0)], lr=4e-3)
    criterion = nn.CrossEntropyLoss(label_smoothing=0.1)
    g = torch.Generator(device=device).manual_seed(1234)
    samples = torch.randn(a.batch, 3, a.res, a.res, device=device, generator=g)
    targets = torch.randint(0, 1000, (a.batch,), device=device, generator=g)
    if a.criterion is not None:
        import slak_amd
        if a.criterion == "label_smoothing":
            criterion = slak_amd.LabelSmoothingCrossEntropy(0.1)
        else:                                                    # a mixup-shaped target, built on the device once: two classes share 0.9, the floor is 0.1 / K
            criterion = slak_amd.SoftTargetCrossEntropy()
            hard = targets
            targets = torch.full((a.batch, 1000), 0.1 / 1000, device=device)
            targets[torch.arange(a.batch, device=device), hard] += 0.9 * 0.7
            targets[torch.arange(a.batch, device=device), hard.flip(0)] += 0.9 * 0.3
    from slak_amd import loss as slak_loss
    mixup_fn = None
    if a.mixup:
        import numpy as np
        from slak_amd import mixup as slak_mixup
        np.random.seed(0)
        mixup_fn = slak_mixup.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=1000)

    loss_scaler = None
    if a.scaler:
        from slak_amd.scaler import NativeScalerWithGradNormCount
        loss_scaler = NativeScalerWithGradNormCount(enabled=False)
    grad_norm = [None]

    def step():
        x, t = (samples, targets) if mixup_fn is None else mixup_fn(samples, hard)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = criterion(model(x), t)
        if loss_scaler is not None:
            grad_norm[0] = loss_scaler(loss, opt, clip_grad=a.clip_grad, parameters=model.parameters())
        else:
            loss.backward()
            if a.clip_grad is not None:
                grad_norm[0] = opt.step_with_grad_norm(clip_grad=a.clip_grad)
            else:
                opt.step()
        opt.zero_grad(set_to_none=True)
        return loss

    model.train()
    for _ in range(a.prime + a.warmup):
        loss = step()
    torch.cuda.synchronize()
    hits0 = getattr(block_ops, "pitched_block_hits", 0)
    rhits0 = getattr(block_ops, "pitched_runner_hits", 0)
    head0, fused0 = block_ops.head_hits, slak_loss.fused_hits
    mix0 = slak_mixup.fused_hits if a.mixup else 0
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    hits = getattr(block_ops, "pitched_block_hits", 0) - hits0
    rhits = getattr(block_ops, "pitched_runner_hits", 0) - rhits0
    head_hits, fused_hits = block_ops.head_hits - head0, slak_loss.fused_hits - fused0
    extra = {"mixup": True, "mixup_hits_per_step": (slak_mixup.fused_hits - mix0) / max(1, a.steps)} if a.mixup else {}
    if grad_norm[0] is not None:
        extra.update({"clip_grad": a.clip_grad, "scaler": bool(a.scaler), "grad_norm": float(grad_norm[0])})
    host = float("inf")
    for _ in range(3):
        h0 = time.perf_counter()
        for _ in range(3):
            step()
        host = min(host, (time.perf_counter() - h0) / 3)
        torch.cuda.synchronize()
    base_dims = (128, 256, 512, 1024) if a.model == "base" else (96, 192, 384, 768)
    dims = [int(d * a.width) for d in base_dims]
    print(json.dumps({"workload": "SLaK-%s 51x51, width_factor %g (C = %s), bs=%d, %dx%d, bf16, MaskedAdamW" % (a.model[0].upper(), a.width, dims, a.batch, a.res, a.res),
                      "ms_per_step": round(1e3 * elapsed / a.steps, 4), "host_enqueue_ms_per_step": round(1e3 * host, 3),
                      "pitched_block_hits": int(hits), "pitched_block_hits_per_step": hits / max(1, a.steps),
                      "pitched_runner_hits_per_step": rhits / max(1, a.steps),
                      "fused_head": bool(a.fused_head), "criterion": a.criterion or "torch", "head_hits_per_step": head_hits / max(1, a.steps),
                      "fused_hits_per_step": fused_hits / max(1, a.steps),
                      "pad_even_widths": bool(getattr(block_ops, "pad_even_widths", False)),
                      "nhwc_pitch": [block_ops.nhwc_pitch(c) if hasattr(block_ops, "nhwc_pitch") else None for c in dims],
                      "block_runner": bool(block_ops._runner() is not None), "steps": a.steps, "warmup": a.warmup, "prime": a.prime,
                      "final_loss": float(loss.item()), "gpu": torch.cuda.get_device_name(0), **extra}), flush=True)


if __name__ == "__main__":
    main()
