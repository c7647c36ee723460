"""Odd / unaligned channel counts on the fused block path (`--width_factor 1.3`: C = 124 / 249 / 499 / 998; pytest -m gpu).

The NCHW tensors keep their logical C; the NHWC intermediates of a block carry a row pitch ldc >= C whose pad columns hold exact zeros, and the
pointwise GEMMs read zero-padded weight copies.  Reference arithmetic = the PyTorch lines of models/SLaK.py:153-166 in fp64 on the same bf16
operands, compared on the logical columns with the tolerances tests/test_block_tail_gpu.py uses for the unpitched ops.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tail_calls import NAN, _close, _ln_bwd_ld, _ln_fwd_ld, _pitched, _sr_bwd_ld, _sr_fwd_ld, _st

pytestmark = pytest.mark.gpu

# (N, C, H, W, ldc): tiny C, the two odd stages on 7 x 7 / 14 x 14 / a plane that is no multiple of 4, the widest odd C, the two even width-1.3 stages,
# an odd C whose four ops all run the pitched LDS-tile kernels (P % 4 == 0 and != 0)
LD_SHAPES = [(2, 5, 3, 3, 64), (2, 249, 7, 7, 256), (3, 249, 14, 14, 256), (2, 499, 7, 7, 512), (2, 499, 4, 6, 512), (1, 1023, 5, 3, 1024),
             (2, 124, 8, 8, 128), (2, 998, 7, 7, 1024), (2, 301, 6, 6, 304), (2, 301, 5, 3, 304)]


# ---- 1. pitched LayerNorm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W,ldc", LD_SHAPES)
def test_pitched_layernorm_matches_layer_norm(N, C, H, W, ldc, gpu):
    from slak_amd import _lib
    L = _lib.lib()
    torch.manual_seed(C + H)
    x = (torch.randn(N, C, H, W, device=gpu) * 2 + 0.3).bfloat16()
    w = torch.randn(C, device=gpu) * 0.5 + 1
    b = torch.randn(C, device=gpu) * 0.1
    g = torch.randn(N, H, W, C, device=gpu).bfloat16()
    y, mean, rstd = _ln_fwd_ld(L, x, w, b, ldc)
    dx, dw, db = _ln_bwd_ld(L, _pitched(g, ldc, NAN), x, w, mean, rstd, ldc)       # the pad columns of g hold NaN: never read
    xr = x.double().requires_grad_(True); wr = w.double().requires_grad_(True); br = b.double().requires_grad_(True)
    yr = F.layer_norm(xr.permute(0, 2, 3, 1), (C,), wr, br, 1e-6)
    yr.backward(g.double())
    assert torch.equal(y[..., C:], torch.zeros_like(y[..., C:])) and not torch.signbit(y[..., C:].float()).any(), "pad columns of y must be +0"
    _close(y[..., :C], yr, 2.0 ** -8 * 1.01, "y")
    mr = x.double().mean(1).reshape(N, H * W)
    # a pad channel in the statistics would move the mean by the factor C / ldc.  fp32: a lane adds <= 16 values, six shuffle steps follow -- at most
    # 22 roundings of 2^-24 on sum|x| / C ~ 1.7, i.e. 2.3e-6 absolute against max |mean| >= 0.3
    _close(mean, mr, 1e-5, "mean over the logical C")
    assert torch.isfinite(dx).all() and torch.isfinite(dw).all() and torch.isfinite(db).all()
    _close(dx, xr.grad, 2.0 ** -8 * 1.5, "dx")
    _close(dw, wr.grad, 1e-4, "dweight")
    _close(db, br.grad, 1e-4, "dbias")
    # the same through the autograd op
    from slak_amd import block_ops
    x2 = x.clone().requires_grad_(True); w2 = w.clone().requires_grad_(True); b2 = b.clone().requires_grad_(True)
    y2 = block_ops.ln_nchw_to_nhwc_pitched(x2, w2, b2, 1e-6, ldc)
    assert y2.shape == (N, H, W, ldc) and torch.equal(y2, y)
    y2.backward(_pitched(g, ldc, NAN))
    assert torch.equal(x2.grad, dx) and torch.equal(w2.grad, dw) and torch.equal(b2.grad, db)


# ---- 2. pitched scale_residual -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W,ldc", LD_SHAPES)
@pytest.mark.parametrize("mode", ["f32", "f32_scale", "bf16", "bf16_scale", "lowp_copy"])
def test_pitched_scale_residual_matches_torch(N, C, H, W, ldc, mode, gpu):
    from slak_amd import _lib
    L = _lib.lib()
    torch.manual_seed(C + W)
    lowp = mode == "lowp_copy"
    sc = torch.randn(N, C, H, W, device=gpu).to(torch.bfloat16 if mode.startswith("bf16") else torch.float32)
    z = torch.randn(N, H, W, C, device=gpu).bfloat16()
    gamma = torch.randn(C, device=gpu) * 0.3
    scale = (torch.rand(N, device=gpu) > 0.3).float() / 0.7 if (lowp or mode.endswith("scale")) else None
    dout = torch.randn(N, C, H, W, device=gpu)
    d16 = torch.randn(N, C, H, W, device=gpu).bfloat16() if lowp else None
    zn, z0 = _pitched(z, ldc, NAN), _pitched(z, ldc, 0.0)
    out, out16 = _sr_fwd_ld(L, sc, zn, gamma, scale, ldc, lowp)
    sn = scale.double().view(N, 1, 1, 1) if scale is not None else 1.0
    ref = sc.double() + (gamma.double() * z.double()).permute(0, 3, 1, 2) * sn
    _close(out, ref, 1e-6, "out")
    assert torch.equal(out, _sr_fwd_ld(L, sc, z0, gamma, scale, ldc, lowp)[0]), "the pad columns of z must not reach the result"
    if lowp:
        assert torch.equal(out16, out.bfloat16())
    dsum, dz, dg, dzc = _sr_bwd_ld(L, dout, d16, zn, gamma, scale, ldc)
    d = dout.double() + (d16.double() if lowp else 0.0)
    if lowp:
        _close(dsum, d, 1e-6, "dshortcut")
    ds = d * sn
    dz_ref = (ds * gamma.double().view(1, C, 1, 1)).permute(0, 2, 3, 1)
    assert torch.equal(dz[..., C:], torch.zeros_like(dz[..., C:])) and not torch.signbit(dz[..., C:].float()).any(), "pad columns of dz must be +0"
    _close(dz[..., :C], dz_ref, 2.0 ** -8 * 1.01, "dz")
    assert torch.isfinite(dg).all() and torch.isfinite(dzc).all()
    _close(dg, (ds.permute(0, 2, 3, 1) * z.double()).sum((0, 1, 2)), 1e-4, "dgamma")
    _close(dzc, dz_ref.sum((0, 1, 2)), 1e-4, "column sums of dz")
    b0 = _sr_bwd_ld(L, dout, d16, z0, gamma, scale, ldc)
    assert torch.equal(b0[1], dz) and torch.equal(b0[2], dg) and torch.equal(b0[3], dzc), "the pad columns of z must not reach the gradients"
    # through block_ops (what the autograd nodes call): pitch read off z
    from slak_amd import block_ops
    with torch.no_grad():
        r = block_ops._scale_residual_fwd(sc, z0, gamma, scale, lowp)
        assert torch.equal(r[0], out)
        bb = block_ops._scale_residual_bwd(z0, gamma, scale, sc.dtype, dout, d16)
        assert bb[1].shape == (N, H, W, ldc) and torch.equal(bb[1], dz) and torch.equal(bb[2], dg) and torch.equal(bb[3], dzc)
        _close(bb[0], d, 2.0 ** -8 * 1.01 if sc.dtype == torch.bfloat16 else 1e-6, "dshortcut")
    with pytest.raises(RuntimeError):
        block_ops.scale_residual(sc, z0, gamma, scale)           # the public op keeps its unpitched contract


# ---- 3. ldc == C is the existing entry point ------------------------------------------------------------------------------------
# (the last three: LDS-tile kernels for every op -- one workgroup per tile with C % 8 != 0, the persistent ones with P % 4 == 0 and != 0)
@pytest.mark.parametrize("N,C,H,W", [(2, 96, 16, 16), (2, 64, 9, 11), (2, 384, 14, 14), (3, 512, 14, 14), (2, 98, 6, 6), (2, 258, 6, 6), (2, 258, 5, 3)])
def test_pitch_equal_to_c_is_the_plain_entry_point_bit_for_bit(N, C, H, W, gpu):
    from slak_amd import _lib, block_ops
    L = _lib.lib()
    torch.manual_seed(C + H)
    x = (torch.randn(N, C, H, W, device=gpu) * 2 + 0.3).bfloat16()
    w = torch.randn(C, device=gpu) * 0.5 + 1; b = torch.randn(C, device=gpu) * 0.1
    g = torch.randn(N, H, W, C, device=gpu).bfloat16()
    y, mean, rstd = _ln_fwd_ld(L, x, w, b, C)
    y0, mean0, rstd0 = block_ops._ln_fwd_impl(x, w, b, 1e-6)
    assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    for a_, b_ in zip((y, mean, rstd), _ln_fwd_ld(L, x, w, b, None)):                    # (None: the plain symbol itself)
        assert torch.equal(a_, b_)
    for a_, b_ in zip(_ln_bwd_ld(L, g, x, w, mean, rstd, C), block_ops._ln_bwd_impl(g, x, w, mean0, rstd0)):
        assert torch.equal(a_, b_)
    for a_, b_ in zip(_ln_bwd_ld(L, g, x, w, mean, rstd, C), _ln_bwd_ld(L, g, x, w, mean, rstd, None)):
        assert torch.equal(a_, b_)
    sc = torch.randn(N, C, H, W, device=gpu); z = torch.randn(N, H, W, C, device=gpu).bfloat16(); gamma = torch.randn(C, device=gpu) * 0.3
    scale = (torch.rand(N, device=gpu) > 0.3).float() / 0.7
    dout = torch.randn(N, C, H, W, device=gpu); d16 = torch.randn(N, C, H, W, device=gpu).bfloat16()
    with torch.no_grad():
        for a_, b_ in zip(_sr_fwd_ld(L, sc, z, gamma, scale, C, True), block_ops._scale_residual_fwd(sc, z, gamma, scale, True)):
            assert torch.equal(a_, b_)
        for a_, b_ in zip(_sr_bwd_ld(L, dout, d16, z, gamma, scale, C), block_ops._scale_residual_bwd(z, gamma, scale, sc.dtype, dout, d16)):
            assert torch.equal(a_, b_)
        for a_, b_ in zip(_sr_fwd_ld(L, sc, z, gamma, scale, C, True) + _sr_bwd_ld(L, dout, d16, z, gamma, scale, C),
                          _sr_fwd_ld(L, sc, z, gamma, scale, None, True) + _sr_bwd_ld(L, dout, d16, z, gamma, scale, None)):
            assert torch.equal(a_, b_)


# ---- 4. zero-padded bf16 weight copies ---------------------------------------------------------------------------------------------
def test_pad_cast_bf16_batch(gpu):
    from slak_amd import _lib
    L = _lib.lib()
    torch.manual_seed(4)
    w = torch.randn(996, 249, device=gpu); bias = torch.randn(996, device=gpu); small = torch.randn(20, 5, device=gpu)
    w[3, 7] = 1e-40; w[5, 5] = -0.0; w[9, 1] = 3.3895313892515355e38                      # denormal, negative zero, rounds to inf
    jobs = [(w, (1024, 256), 0), (w, (256, 1024), 1), (bias.view(1, 996), (1, 1024), 0), (small, (256, 64), 0), (small, (64, 256), 1)]
    dsts = [torch.full(shape, NAN, dtype=torch.bfloat16, device=gpu) for _, shape, _ in jobs]
    n = len(jobs)
    vp, ci = ctypes.c_void_p * n, ctypes.c_int * n
    _lib.check(L.slak_pad_cast_bf16_batch(vp(*[s.data_ptr() for s, _, _ in jobs]), vp(*[d.data_ptr() for d in dsts]),
                                          ci(*[s.shape[0] for s, _, _ in jobs]), ci(*[s.shape[1] for s, _, _ in jobs]),
                                          ci(*[sh[0] for _, sh, _ in jobs]), ci(*[sh[1] for _, sh, _ in jobs]), ci(*[tr for _, _, tr in jobs]),
                                          n, _st(gpu)), "slak_pad_cast_bf16_batch")
    for (s, shape, tr), d in zip(jobs, dsts):
        ref = s.bfloat16().t() if tr else s.bfloat16()
        ref = F.pad(ref, (0, shape[1] - ref.shape[1], 0, shape[0] - ref.shape[0]))
        assert torch.equal(d.view(torch.int16), ref.contiguous().view(torch.int16)), (tuple(s.shape), shape, tr)


# ---- 5. the MLP on pitched operands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,C,pad_even", [(2, 7, 7, 249, False), (2, 14, 14, 499, False), (2, 7, 7, 5, False), (2, 7, 7, 124, True)])
def test_padded_mlp_matches_torch(N, H, W, C, pad_even, gpu):
    """mlp_scale_residual on pitched t (M = N*H*W rows of ldc): z, dt and the four parameter gradients vs fp64 on the same rounded operands
    (shortcut 0, gamma 1: `out` IS z)."""
    from slak_amd import block_ops
    saved = (block_ops.pad_even_widths, block_ops.cache_lowp_weights)
    try:
        block_ops.pad_even_widths = pad_even
        block_ops.cache_lowp_weights = False
        ldc = block_ops.nhwc_pitch(C)
        assert ldc != C and ldc % 64 == 0
        torch.manual_seed(N * H * W)
        t0 = torch.randn(N, H, W, C, device=gpu).bfloat16()
        t = _pitched(t0, ldc, 0.0).requires_grad_(True)
        w1 = (torch.randn(4 * C, C, device=gpu) * 0.05).requires_grad_(True); b1 = (torch.randn(4 * C, device=gpu) * 0.05).requires_grad_(True)
        w2 = (torch.randn(C, 4 * C, device=gpu) * 0.05).requires_grad_(True); b2 = (torch.randn(C, device=gpu) * 0.05).requires_grad_(True)
        gamma = torch.ones(C, device=gpu, requires_grad=True)
        sc = torch.zeros(N, C, H, W, device=gpu)
        dout = torch.randn(N, C, H, W, device=gpu).bfloat16().float()
        h0 = block_ops.pitched_block_hits
        out = block_ops.mlp_scale_residual(sc, t, w1, b1, w2, b2, gamma)
        assert block_ops.pitched_block_hits == h0 + 1
        out.backward(dout)
        td = t0.double().requires_grad_(True)
        ps = [p.detach().bfloat16().double().requires_grad_(True) for p in (w1, b1, w2, b2)]
        zr = F.linear(F.gelu(F.linear(td, ps[0], ps[1])), ps[2], ps[3])
        zr.backward(dout.double().permute(0, 2, 3, 1))
        _close(out.permute(0, 2, 3, 1), zr, 1.5e-2, "z")
        assert torch.equal(t.grad[..., C:], torch.zeros_like(t.grad[..., C:]))
        _close(t.grad[..., :C], td.grad, 2e-2, "dt")
        for got, ref, p, n in ((w1.grad, ps[0].grad, w1, "dw1"), (b1.grad, ps[1].grad, b1, "db1"), (w2.grad, ps[2].grad, w2, "dw2"),
                               (b2.grad, ps[3].grad, b2, "db2")):
            assert got.shape == p.shape and got.is_contiguous() and got.dtype == torch.float32, n
            _close(got, ref, 2e-2, n)
    finally:
        block_ops.pad_even_widths, block_ops.cache_lowp_weights = saved


# ---- 6. a whole Block at odd C ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,shape", [(249, (2, 249, 14, 14)), (25, (3, 25, 9, 11))])
def test_block_at_odd_width_matches_reference_composition(C, shape, gpu):
    """Block under bf16 autocast: fused tail and the whole block as one node against the reference's op sequence; both must run pitched."""
    import slak_amd.slak_model as M
    from slak_amd import block_ops
    saved = (M.Block.fused_tail, M.ReparamLargeKernelConv.fused_bn, M.ReparamLargeKernelConv.fused_tri, M.Block.fused_block)
    M.use_sync_bn = False
    try:
        torch.manual_seed(0)
        blk = M.Block(C, drop_path=0.0, layer_scale_init_value=0.5, kernel_size=(13, 5), Decom=True, bn=True, lowp_dwconv=True).to(gpu)
        with torch.no_grad():
            blk.gamma.uniform_(0.2, 0.8)
        x = torch.randn(*shape, device=gpu)
        dy = torch.randn_like(x)
        outs = {}
        for mode in ("reference", "tail", "block"):
            M.Block.fused_tail = mode != "reference"
            M.ReparamLargeKernelConv.fused_bn = M.ReparamLargeKernelConv.fused_tri = M.Block.fused_block = mode == "block"
            blk.zero_grad()
            for bn in (blk.large_kernel.LoRA1.bn, blk.large_kernel.LoRA2.bn, blk.large_kernel.small_conv.bn):
                bn.reset_running_stats()
            xi = x.clone().requires_grad_(True)
            h0 = getattr(block_ops, "pitched_block_hits")
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = blk(xi)
            y.backward(dy)
            assert block_ops.pitched_block_hits - h0 == (0 if mode == "reference" else 1), mode
            outs[mode] = (y.detach(), xi.grad.detach(), blk.gamma.grad.clone(), blk.norm.weight.grad.clone(), blk.norm.bias.grad.clone(),
                          blk.pwconv1.weight.grad.clone(), blk.pwconv2.weight.grad.clone(), blk.large_kernel.LoRA1.conv.weight.grad.clone(),
                          blk.pwconv2.bias.grad.clone(), blk.pwconv1.bias.grad.clone())
        names = ("y", "dx", "dgamma", "dnorm.weight", "dnorm.bias", "dpwconv1.weight", "dpwconv2.weight", "dLoRA1.weight", "dpwconv2.bias", "dpwconv1.bias")
        for mode in ("tail", "block"):
            for a, b, n in zip(outs[mode], outs["reference"], names):
                assert a.dtype == b.dtype and a.shape == b.shape and a.is_contiguous(), (mode, n)
                _close(a, b, 3e-2, "%s (%s)" % (n, mode))           # two bf16 pipelines with different rounding points
    finally:
        (M.Block.fused_tail, M.ReparamLargeKernelConv.fused_bn, M.ReparamLargeKernelConv.fused_tri, M.Block.fused_block) = saved


# ---- 7. a small odd-width model ------------------------------------------------------------------------------------------------------
def test_small_odd_width_model_trains_like_the_unfused_one(gpu):
    """Three MaskedAdamW + Masking steps, every fused path on against every fused path off; the padded weight copies follow the optimizer
    and the masks."""
    import contextlib, copy, io, types
    import slak_amd.slak_model as M
    from slak_amd import block_ops
    from slak_amd.optim_factory import MaskedAdamW
    from slak_amd.sparse_core import CosineDecay, Masking
    saved = (M.Block.fused_tail, M.ReparamLargeKernelConv.fused_bn, M.ReparamLargeKernelConv.fused_tri, M.Block.fused_block, M.LayerNorm.fused_cf,
             block_ops.cache_lowp_weights)
    M.use_sync_bn = False
    try:
        torch.manual_seed(3)
        net0 = M.SLaK(in_chans=3, num_classes=10, depths=[1, 1, 2, 1], dims=[10, 21, 43, 86], drop_path_rate=0.0, kernel_size=[13, 13, 9, 7, 5],
                      Decom=True, bn=True, lowp_dwconv=True).to(gpu)
        g = torch.Generator(device=gpu).manual_seed(11)
        xs = torch.randn(4, 3, 64, 64, device=gpu, generator=g); ys = torch.randint(0, 10, (4,), device=gpu, generator=g)
        losses = {}
        for fused in (False, True):
            M.Block.fused_tail = M.ReparamLargeKernelConv.fused_bn = M.ReparamLargeKernelConv.fused_tri = M.Block.fused_block = fused
            M.LayerNorm.fused_cf = fused
            block_ops.cache_lowp_weights = fused
            net = copy.deepcopy(net0)
            torch.manual_seed(17)                                     # the same random masks in both runs (Masking draws them from the global generator)
            opt = MaskedAdamW(net.parameters(), lr=1e-3)
            margs = types.SimpleNamespace(device=str(gpu), fix=False, update_frequency=2, only_L=False, sparse_init="uniform", sparsity=0.4, distributed=False)
            with contextlib.redirect_stdout(io.StringIO()):
                mask = Masking(opt, None, CosineDecay(0.3, 100), prune_rate=0.3, prune_mode="magnitude", growth_mode="gradient",
                               redistribution_mode="none", args=margs)
                mask.add_module(net)
            h0 = block_ops.pitched_block_hits
            ls = []
            for it in range(3):
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    loss = F.cross_entropy(net(xs).float(), ys)
                loss.backward()
                with contextlib.redirect_stdout(io.StringIO()):
                    mask.step()
                opt.zero_grad(set_to_none=True)
                ls.append(float(loss.item()))
                if fused:
                    block_ops.refresh_padded()                        # (what the first pitched block of the next step does)
                    mine = {id(p): n for n, p in net.named_parameters()}
                    seen = masked = 0
                    for p, c, tr in block_ops.padded_cache_entries():
                        if id(p) not in mine:
                            continue
                        seen += 1
                        src = p.detach().bfloat16()
                        src = src.view(1, -1) if src.dim() == 1 else (src.t() if tr else src)
                        c2 = c.view(1, -1) if c.dim() == 1 else c
                        ref = F.pad(src, (0, c2.shape[1] - src.shape[1], 0, c2.shape[0] - src.shape[0]))
                        assert torch.equal(c2, ref), (mine[id(p)], tr, it)
                        mk = mask.masks.get(mine[id(p)])
                        if mk is not None:
                            masked += 1
                            mk2 = mk.t() if tr else mk
                            assert (c2[:mk2.shape[0], :mk2.shape[1]][mk2 == 0] == 0).all(), (mine[id(p)], "masked entries")
                    assert seen == 6 * 3                               # three pitched blocks (C = 21, 43, 43), six copies each
                    assert masked == 4 * 3                             # ... of them the two weights in both orientations carry a mask
            assert block_ops.pitched_block_hits - h0 == (9 if fused else 0)
            losses[fused] = ls
        assert all(l == l for l in losses[True])
        for a, b in zip(losses[True], losses[False]):
            assert abs(a - b) <= 3e-2 * abs(b), (losses[True], losses[False])
    finally:
        (M.Block.fused_tail, M.ReparamLargeKernelConv.fused_bn, M.ReparamLargeKernelConv.fused_tri, M.Block.fused_block, M.LayerNorm.fused_cf,
         block_ops.cache_lowp_weights) = saved


# ---- 8. the branch BatchNorms at odd C (guard) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W", [(3, 249, 7, 7), (4, 25, 9, 11)])
def test_branch_bn3_at_odd_width(N, C, H, W, gpu):
    import copy
    import torch.nn as nn
    from slak_amd import block_ops
    torch.manual_seed(C + H)
    bns = [nn.BatchNorm2d(C).to(gpu) for _ in range(3)]
    for bn in bns:
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.3, 0.3)
            bn.running_mean.uniform_(-0.2, 0.2); bn.running_var.uniform_(0.5, 2.0)
    refs = [copy.deepcopy(bn).double() for bn in bns]
    ys = [((torch.randn(N, C, H, W, device=gpu) * (1 + i) + 0.1 * i).bfloat16()).requires_grad_(True) for i in range(3)]
    dout = torch.randn(N, C, H, W, device=gpu).bfloat16()
    out = block_ops.branch_bn3(ys[0], ys[1], ys[2], *bns)
    out.backward(dout)
    yr = [y.detach().double().requires_grad_(True) for y in ys]
    outr = refs[0](yr[0]) + refs[1](yr[1]) + refs[2](yr[2])
    outr.backward(dout.double())
    _close(out, outr, 2.0 ** -8 * 1.05, "out")
    for i in range(3):
        _close(ys[i].grad, yr[i].grad, 2.0 ** -8 * 1.5, "dy%d" % i)
        _close(bns[i].weight.grad, refs[i].weight.grad, 2e-4, "dgamma%d" % i)
        _close(bns[i].bias.grad, refs[i].bias.grad, 2e-4, "dbeta%d" % i)
        _close(bns[i].running_mean, refs[i].running_mean, 1e-5, "running_mean%d" % i)
        _close(bns[i].running_var, refs[i].running_var, 1e-5, "running_var%d" % i)
