"""The C++ block runner on pitched blocks (odd C of the width-1.3 models, or an even width under `pad_even_widths`; pytest -m gpu).

The runner issues the launches of block_ops._BlockFn's Python sequence on the same operands -- the convs and BatchNorms on the logical C, the MLP
on the zero-padded operands of pitch ldc, the tail through the `slak_*_ld` entry points -- so outputs, every gradient and the running statistics
must be bit-identical with and without it.  `block_ops.pitched_runner_hits` counts the pitched block forwards the runner issued,
`pitched_block_hits` counts them whoever issued them.
"""
import contextlib
import copy
import io
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture
def fused(gpu):
    """Every fused path on (the whole block as one autograd node), restored afterwards; skips without the runner module."""
    import slak_amd.slak_model as M
    from slak_amd import block_ops
    if block_ops._runner() is None:
        pytest.skip("block runner module not built")
    saved = (M.Block.fused_tail, M.ReparamLargeKernelConv.fused_bn, M.ReparamLargeKernelConv.fused_tri, M.Block.fused_block, M.LayerNorm.fused_cf,
             block_ops.cache_lowp_weights, block_ops.pad_even_widths, block_ops._runner_mod)
    M.use_sync_bn = False
    M.Block.fused_tail = M.ReparamLargeKernelConv.fused_bn = M.ReparamLargeKernelConv.fused_tri = M.Block.fused_block = True
    try:
        yield block_ops
    finally:
        (M.Block.fused_tail, M.ReparamLargeKernelConv.fused_bn, M.ReparamLargeKernelConv.fused_tri, M.Block.fused_block, M.LayerNorm.fused_cf,
         block_ops.cache_lowp_weights, block_ops.pad_even_widths, block_ops._runner_mod) = saved


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()


def _bns(blk):
    return (blk.large_kernel.LoRA1.bn, blk.large_kernel.LoRA2.bn, blk.large_kernel.small_conv.bn)


def _run_block(blk, x0, dy, dy16, emit):
    """One forward and backward of the block under bf16 autocast -> everything a training step would see."""
    blk.zero_grad(set_to_none=True)
    for bn in _bns(blk):
        bn.reset_running_stats()
    blk.emit_lowp = emit
    x = x0.clone().requires_grad_(True)
    torch.manual_seed(23)                                       # the drop-path draw (sample_scale)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y, y16 = blk.forward_pair(x, None)
    assert (y16 is not None) == emit
    loss = (y * dy).sum()
    if emit:
        loss = loss + (y16.float() * dy16).sum()
    loss.backward()
    res = {"y": _np(y), "dx": _np(x.grad)}
    assert x.grad.dtype == x0.dtype and x.grad.is_contiguous()
    if emit:
        res["y16"] = _np(y16)
    for n, p in blk.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32 and p.grad.is_contiguous(), n
        res["d" + n] = _np(p.grad)
    for i, bn in enumerate(_bns(blk)):
        res["running_mean%d" % i] = _np(bn.running_mean); res["running_var%d" % i] = _np(bn.running_var)
    return res


def _runner_against_python(block_ops, gpu, C, shape, pitched=True):
    import slak_amd.slak_model as M
    torch.manual_seed(C)
    blk = M.Block(C, drop_path=0.2, layer_scale_init_value=0.5, kernel_size=(13, 5), Decom=True, bn=True, lowp_dwconv=True).to(gpu)
    blk.train()
    with torch.no_grad():
        blk.gamma.uniform_(0.2, 0.8)
    x32 = torch.randn(*shape, device=gpu)
    dy = torch.randn(*shape, device=gpu); dy16 = torch.randn(*shape, device=gpu)
    runner = block_ops._runner_mod
    for xdt in (torch.float32, torch.bfloat16):
        for emit in (False, True):
            x0 = x32.to(xdt)
            block_ops._runner_mod = runner
            hb, hr = block_ops.pitched_block_hits, block_ops.pitched_runner_hits
            with_runner = _run_block(blk, x0, dy, dy16, emit)
            assert block_ops.pitched_runner_hits - hr == (1 if pitched else 0), "the runner declined the block"
            assert block_ops.pitched_block_hits - hb == (1 if pitched else 0)
            block_ops._runner_mod = None
            hb, hr = block_ops.pitched_block_hits, block_ops.pitched_runner_hits
            try:
                python = _run_block(blk, x0, dy, dy16, emit)
            finally:
                block_ops._runner_mod = runner
            assert block_ops.pitched_runner_hits == hr and block_ops.pitched_block_hits - hb == (1 if pitched else 0)
            assert sorted(with_runner) == sorted(python)
            bad = [k for k in python if with_runner[k].shape != python[k].shape or not np.array_equal(with_runner[k], python[k])]
            assert not bad, (str(xdt), emit, bad)
            assert all(np.isfinite(v).all() for v in python.values())


# 14 x 14 and 7 x 7: the small-plane tail kernels (`chan`, `chan1`); 28 x 28: the pixel-pair `LD` kernels
@pytest.mark.parametrize("C,shape", [(249, (2, 249, 14, 14)), (499, (2, 499, 7, 7)), (499, (2, 499, 14, 14)), (249, (2, 249, 28, 28))])
def test_runner_issues_a_pitched_block_like_the_python_sequence(C, shape, fused, gpu):
    _runner_against_python(fused, gpu, C, shape)


def test_runner_takes_an_even_width_under_pad_even_widths(fused, gpu):
    fused.pad_even_widths = True
    assert fused.nhwc_pitch(124) == 128
    _runner_against_python(fused, gpu, 124, (2, 124, 8, 8))


def test_width_one_block_is_not_a_pitched_block(fused, gpu):
    assert fused.nhwc_pitch(96) == 96
    _runner_against_python(fused, gpu, 96, (2, 96, 14, 14), pitched=False)


def test_small_odd_width_model_trains_the_same_with_and_without_the_runner(fused, gpu):
    """Three MaskedAdamW + Masking steps with every fused path on: losses and all parameters bit-identical, nine pitched blocks issued by the runner."""
    import slak_amd.slak_model as M
    from slak_amd.optim_factory import MaskedAdamW
    from slak_amd.sparse_core import CosineDecay, Masking
    block_ops = fused
    M.LayerNorm.fused_cf = True
    block_ops.cache_lowp_weights = True
    torch.manual_seed(3)
    net0 = M.SLaK(in_chans=3, num_classes=10, depths=[1, 1, 2, 1], dims=[10, 21, 43, 86], drop_path_rate=0.0, kernel_size=[13, 13, 9, 7, 5],
                  Decom=True, bn=True, lowp_dwconv=True).to(gpu)
    g = torch.Generator(device=gpu).manual_seed(11)
    xs = torch.randn(4, 3, 64, 64, device=gpu, generator=g); ys = torch.randint(0, 10, (4,), device=gpu, generator=g)
    runner = block_ops._runner_mod
    out = {}
    for use in (True, False):
        block_ops._runner_mod = runner if use else None
        try:
            net = copy.deepcopy(net0)
            torch.manual_seed(17)                                     # the same random masks in both runs
            opt = MaskedAdamW(net.parameters(), lr=1e-3)
            margs = types.SimpleNamespace(device=str(gpu), fix=False, update_frequency=2, only_L=False, sparse_init="uniform", sparsity=0.4, distributed=False)
            with contextlib.redirect_stdout(io.StringIO()):
                mask = Masking(opt, None, CosineDecay(0.3, 100), prune_rate=0.3, prune_mode="magnitude", growth_mode="gradient",
                               redistribution_mode="none", args=margs)
                mask.add_module(net)
            hb, hr = block_ops.pitched_block_hits, block_ops.pitched_runner_hits
            losses = []
            for _ in range(3):
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    loss = F.cross_entropy(net(xs).float(), ys)
                loss.backward()
                with contextlib.redirect_stdout(io.StringIO()):
                    mask.step()
                opt.zero_grad(set_to_none=True)
                losses.append(float(loss.item()))
            assert block_ops.pitched_block_hits - hb == 9             # three pitched blocks (C = 21, 43, 43), three steps
            assert block_ops.pitched_runner_hits - hr == (9 if use else 0)
            out[use] = (losses, {n: _np(p) for n, p in net.state_dict().items()})
        finally:
            block_ops._runner_mod = runner
    assert all(l == l for l in out[True][0]) and out[True][0] == out[False][0], (out[True][0], out[False][0])
    bad = [n for n in out[False][1] if not np.array_equal(out[True][1][n], out[False][1][n])]
    assert not bad, bad[:5]
