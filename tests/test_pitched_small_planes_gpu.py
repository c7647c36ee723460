"""The small-plane block-tail kernels (`*_chan_kernel`: even planes of at most 256 pixels, a wave per image and channel group; `*_chan1_kernel`:
odd planes, one pixel per lane) behind the pitched entry points `slak_*_ld` (pytest -m gpu).

The channel groups tile the pitch, so a wave's group may be partly or wholly pad columns; its live channel count bounds the channel loops.
Reference arithmetic and tolerances are those of tests/test_odd_width_gpu.py: fp64 `F.layer_norm` / the residual formula on the same bf16
operands, NaN in every pad column of g and z, every output buffer pre-filled with NaN.  Each check first asks slak_block_tail_family that
the call does run the family under test -- on the LDS-tile or pixel-pair kernels the numbers alone would pass and show nothing.
"""
import pytest
import torch
import torch.nn.functional as F

from tail_calls import NAN, _close, _ln_bwd_ld, _ln_fwd_ld, _pitched, _sr_bwd_ld, _sr_fwd_ld

pytestmark = pytest.mark.gpu

LN_FWD, LN_BWD, SR_FWD, SR_BWD = 0, 1, 2, 3
REG, CHAN, CHAN1 = 2, 3, 4
# (N, C, H, W, ldc)
CHAN_SHAPES = [
    (2, 499, 14, 14, 512),      # a partly live last group (19 of 32, 51 of 64)
    (2, 249, 14, 14, 256),
    (3, 449, 6, 6, 512),        # one group with a single live row (32 per wave) and one wholly padded; N = 3: a ragged last workgroup of four waves
    (1, 499, 2, 1, 512),        # one pixel pair: 63 idle lanes
    (2, 193, 14, 14, 256),      # the live channels end in the first third of the last-but-one group of 32
    (5, 249, 14, 14, 256),      # more images than the four waves of a workgroup
]
CHAN1_SHAPES = [
    (2, 499, 7, 7, 512),
    (2, 998, 7, 7, 1024),       # 16 waves in the LayerNorm kernels
    (2, 449, 5, 5, 512),        # a wholly padded group that must still meet the workgroup barriers
    (1, 499, 1, 3, 512),        # three pixels
]
SHAPES = CHAN_SHAPES + CHAN1_SHAPES


def _family(L, op, dt, N, C, P, ldc):
    return int(L.slak_block_tail_family(op, dt, N, C, P, ldc))


@pytest.mark.parametrize("N,C,H,W,ldc", SHAPES)
def test_pitched_layernorm_on_small_planes(N, C, H, W, ldc, gpu):
    from slak_amd import _lib
    L = _lib.lib()
    P = H * W
    want = CHAN1 if P & 1 else CHAN
    # the backward runs the family under test on every shape; the forward has no `chan` kernel (even planes stay where they were)
    assert _family(L, LN_BWD, 0, N, C, P, ldc) == want
    if P & 1:
        assert _family(L, LN_FWD, 0, N, C, P, ldc) == CHAN1
    torch.manual_seed(C + H)
    x = (torch.randn(N, C, H, W, device=gpu) * 2 + 0.3).bfloat16()
    w = torch.randn(C, device=gpu) * 0.5 + 1
    b = torch.randn(C, device=gpu) * 0.1
    g = torch.randn(N, H, W, C, device=gpu).bfloat16()
    gn, g0 = _pitched(g, ldc, NAN), _pitched(g, ldc, 0.0)
    y, mean, rstd = _ln_fwd_ld(L, x, w, b, ldc)
    dx, dw, db = _ln_bwd_ld(L, gn, x, w, mean, rstd, ldc)                 # the pad columns of g hold NaN: never taken into a sum
    xr = x.double().requires_grad_(True); wr = w.double().requires_grad_(True); br = b.double().requires_grad_(True)
    yr = F.layer_norm(xr.permute(0, 2, 3, 1), (C,), wr, br, 1e-6)
    yr.backward(g.double())
    assert torch.equal(y[..., C:], torch.zeros_like(y[..., C:])) and not torch.signbit(y[..., C:].float()).any(), "pad columns of y must be +0"
    _close(y[..., :C], yr, 2.0 ** -8 * 1.01, "y")
    _close(mean, x.double().mean(1).reshape(N, P), 1e-5, "mean over the logical C")
    assert torch.isfinite(rstd).all() and torch.isfinite(dx).all() and torch.isfinite(dw).all() and torch.isfinite(db).all()
    _close(dx, xr.grad, 2.0 ** -8 * 1.5, "dx")
    _close(dw, wr.grad, 1e-4, "dweight")
    _close(db, br.grad, 1e-4, "dbias")
    again = _ln_bwd_ld(L, g0, x, w, mean, rstd, ldc)
    assert torch.equal(again[0], dx) and torch.equal(again[1], dw) and torch.equal(again[2], db), "pad columns of g must not reach a result; fixed-order sums"
    again = _ln_bwd_ld(L, gn, x, w, mean, rstd, ldc)
    assert torch.equal(again[1], dw) and torch.equal(again[2], db), "a second call must give the same bits"


@pytest.mark.parametrize("N,C,H,W,ldc", SHAPES)
@pytest.mark.parametrize("mode", ["f32", "f32_scale", "bf16", "bf16_scale", "lowp_copy"])
def test_pitched_scale_residual_on_small_planes(N, C, H, W, ldc, mode, gpu):
    from slak_amd import _lib
    L = _lib.lib()
    P = H * W
    want = CHAN1 if P & 1 else CHAN
    bf16_sc = mode.startswith("bf16")
    assert _family(L, SR_BWD, 0, N, C, P, ldc) == want
    if not bf16_sc:                                                       # a bf16 shortcut has no small-plane kernel: it must pass on whatever runs
        assert _family(L, SR_FWD, _lib.SLAK_F32, N, C, P, ldc) == want
    else:
        assert _family(L, SR_FWD, _lib.SLAK_BF16, N, C, P, ldc) not in (0, CHAN, CHAN1)
    torch.manual_seed(C + W)
    lowp = mode == "lowp_copy"
    sc = torch.randn(N, C, H, W, device=gpu).to(torch.bfloat16 if bf16_sc else torch.float32)
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
    b1 = _sr_bwd_ld(L, dout, d16, zn, gamma, scale, ldc)
    assert torch.equal(b1[2], dg) and torch.equal(b1[3], dzc), "a second call must give the same bits"
