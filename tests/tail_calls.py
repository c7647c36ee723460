"""What the GPU tests of the pitched block tail share (test_odd_width_gpu.py, test_pitched_small_planes_gpu.py): the comparison, the pitched
operands and the four ops called through the C ABI on NaN-filled outputs.  `ldc`: the row pitch handed to the `slak_*_ld` symbol; None: the plain
symbol (rows of C)."""
import torch

NAN = float("nan")


def _close(a, b, rel, what):
    a, b = a.double(), b.double()
    err = (a - b).abs().max().item()
    scale = max(1e-6, b.abs().max().item())
    assert err <= rel * scale, "%s: err %.3e vs scale %.3e" % (what, err, scale)


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _ws(L, N, ldc, P, dev):
    nb = int(L.slak_block_tail_workspace_bytes(N, ldc, P))
    return torch.empty(nb, dtype=torch.uint8, device=dev), nb


def _pitched(t, ldc, fill):
    """(..., C) -> (..., ldc) with `fill` in the pad columns"""
    out = torch.full(t.shape[:-1] + (ldc,), fill, dtype=t.dtype, device=t.device)
    out[..., :t.shape[-1]] = t
    return out


def _sym(L, name, C, ldc):
    """-> (the entry point, the pitch of its NHWC tensors, its arguments behind the stream)"""
    return (getattr(L, name), C, ()) if ldc is None else (getattr(L, name + "_ld"), ldc, (ldc,))


def _ln_fwd_ld(L, x, w, b, ldc, eps=1e-6):
    from slak_amd import _lib
    N, C, H, W = x.shape
    fn, ldc, tail = _sym(L, "slak_ln_nchw_to_nhwc_forward", C, ldc)
    y = torch.full((N, H, W, ldc), NAN, dtype=torch.bfloat16, device=x.device)
    mean = torch.full((N, H * W), NAN, device=x.device); rstd = torch.full((N, H * W), NAN, device=x.device)
    _lib.check(fn(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), N, C, H * W, eps, _st(x.device), *tail), "ln fwd ld")
    return y, mean, rstd


def _ln_bwd_ld(L, g, x, w, mean, rstd, ldc):
    from slak_amd import _lib
    N, C, H, W = x.shape
    fn, ldc, tail = _sym(L, "slak_ln_nchw_to_nhwc_backward", C, ldc)
    dx = torch.full_like(x, NAN); dw = torch.full((C,), NAN, device=x.device); db = torch.full((C,), NAN, device=x.device)
    ws, nb = _ws(L, N, ldc, H * W, x.device)
    _lib.check(fn(g.data_ptr(), x.data_ptr(), w.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), N, C, H * W,
                  ws.data_ptr(), nb, _st(x.device), *tail), "ln bwd ld")
    return dx, dw, db


def _sr_fwd_ld(L, sc, z, gamma, scale, ldc, lowp):
    from slak_amd import _lib
    N, C, H, W = sc.shape
    fn, ldc, tail = _sym(L, "slak_scale_residual_forward", C, ldc)
    out = torch.full((N, C, H, W), NAN, device=sc.device)
    out16 = torch.full((N, C, H, W), NAN, dtype=torch.bfloat16, device=sc.device) if lowp else None
    sdt = _lib.SLAK_F32 if sc.dtype == torch.float32 else _lib.SLAK_BF16
    _lib.check(fn(sc.data_ptr(), sdt, z.data_ptr(), gamma.data_ptr(), scale.data_ptr() if scale is not None else None,
                  out.data_ptr(), out16.data_ptr() if lowp else None, N, C, H * W, _st(sc.device), *tail), "sr fwd ld")
    return out, out16


def _sr_bwd_ld(L, dout, d16, z, gamma, scale, ldc):
    from slak_amd import _lib
    N, C, H, W = dout.shape
    fn, ldc, tail = _sym(L, "slak_scale_residual_backward", C, ldc)
    dz = torch.full((N, H, W, ldc), NAN, dtype=torch.bfloat16, device=dout.device)
    dsum = torch.full_like(dout, NAN) if d16 is not None else None
    dg = torch.full((C,), NAN, device=dout.device); dzc = torch.full((C,), NAN, device=dout.device)
    ws, nb = _ws(L, N, ldc, H * W, dout.device)
    _lib.check(fn(dout.data_ptr(), d16.data_ptr() if d16 is not None else None, dsum.data_ptr() if dsum is not None else None,
                  z.data_ptr(), gamma.data_ptr(), scale.data_ptr() if scale is not None else None, dz.data_ptr(),
                  dg.data_ptr(), dzc.data_ptr(), N, C, H * W, ws.data_ptr(), nb, _st(dout.device), *tail), "sr bwd ld")
    return dsum, dz, dg, dzc
