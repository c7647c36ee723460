"""What the GPU tests of the three-branch and pair depthwise-conv launches share (test_fused_launches_gpu.py, ab_switches.py): the two bounds
against the C oracle on the rounded operands and the entry points called through the C ABI.  A helper answers None where the matching size or
support query says that the launch does not exist for the shape."""
import ctypes

import numpy as np
import torch


def _L():
    from slak_amd import _lib
    return _lib


def _st(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dt(dtype):
    L = _L()
    return L.SLAK_BF16 if dtype == torch.bfloat16 else L.SLAK_F16


def _r(t, dtype):
    return t.to(dtype).float().cpu().numpy()


def _filters(C, K, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [(torch.randn(C, 1, kh, kw, generator=g) * 0.05).to(dev) for kh, kw in ((K, 5), (5, K), (5, 5))]


def _check_lowp(got, ref, dtype, what):
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    got = got.detach().double().cpu().numpy()
    scale = max(1.0, float(np.abs(ref).max()))
    err = np.abs(got - ref)
    assert err.max() <= 1e-2 * scale, "%s: max err %.3e (scale %.3e)" % (what, err.max(), scale)      # north star, bf16
    bound = ulp * np.abs(ref) + 5e-6 * scale                                                        # half an output ulp + accumulation
    assert (err <= bound).all(), "%s: exceeds the rounding bound by %.3e" % (what, float((err - bound).max()))


def _check_dw(got, ref, n_terms, what):
    """fp32 accumulation of n_terms products: 1e-5 of the largest gradient for short sums, growing with sqrt(n_terms), and never looser than the rtol 1e-4 the
    reference's own test allows a weight gradient (test_correctness.py:67-90) -- the stage-1 sums (401,408 terms) are held to that."""
    err = np.abs(got.double().cpu().numpy() - ref).max()
    assert err <= min(1e-4, 1e-5 * max(1.0, n_terms ** 0.5 / 30)) * max(1.0, np.abs(ref).max()), "%s: %.3e" % (what, err)


def _pair_wgrad(dyv, dys, x, K):
    L = _L(); lib = L.lib()
    N, C, H, W = x.shape
    dt = _dt(x.dtype)
    nb = int(lib.slak_dwconv2d_pair_filter_workspace_bytes(dt, N, C, H, W, K))
    if nb == 0:
        return None
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    dwv = torch.empty(C, 1, K, 5, dtype=torch.float32, device=x.device)
    dws = torch.empty(C, 1, 5, 5, dtype=torch.float32, device=x.device)
    L.check(lib.slak_dwconv2d_pair_backward_filter(dyv.data_ptr(), dys.data_ptr(), x.data_ptr(), dwv.data_ptr(), dws.data_ptr(), dt,
                                                   N, C, H, W, K, ws.data_ptr(), nb, _st(x.device)), "pair_backward_filter")
    return dwv, dws


def _tri_fwd(x, ws, K, stats=False):
    L = _L(); lib = L.lib()
    N, C, H, W = x.shape
    dt = _dt(x.dtype)
    ys = [torch.empty_like(x) for _ in range(3)]
    if stats:
        rows = int(lib.slak_dwconv2d_tri_stats_rows(dt, N, C, H, W, K))
        if rows <= 0:
            return None, None
        st = torch.zeros(rows, C, 6, dtype=torch.float32, device=x.device)
        L.check(lib.slak_dwconv2d_tri_forward_stats(x.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr(), ys[0].data_ptr(),
                                                    ys[1].data_ptr(), ys[2].data_ptr(), st.data_ptr(), dt, N, C, H, W, K, _st(x.device)), "tri_forward_stats")
        return ys, st
    L.check(lib.slak_dwconv2d_tri_forward(x.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr(), ys[0].data_ptr(),
                                          ys[1].data_ptr(), ys[2].data_ptr(), dt, N, C, H, W, K, _st(x.device)), "tri_forward")
    return ys, None


def _tri_dgrad(dys, ws, K):
    L = _L(); lib = L.lib()
    N, C, H, W = dys[0].shape
    dx = torch.empty_like(dys[0])
    L.check(lib.slak_dwconv2d_tri_backward_data(dys[0].data_ptr(), dys[1].data_ptr(), dys[2].data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(),
                                                ws[2].data_ptr(), dx.data_ptr(), _dt(dx.dtype), N, C, H, W, K, _st(dx.device)), "tri_backward_data")
    return dx


def _tri_wgrad(dys, x, K):
    L = _L(); lib = L.lib()
    N, C, H, W = x.shape
    dt = _dt(x.dtype)
    nb = int(lib.slak_dwconv2d_tri_filter_workspace_bytes(dt, N, C, H, W, K))
    if nb == 0:
        return None
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    dws = [torch.empty(C, 1, kh, kw, dtype=torch.float32, device=x.device) for kh, kw in ((K, 5), (5, K), (5, 5))]
    L.check(lib.slak_dwconv2d_tri_backward_filter(dys[0].data_ptr(), dys[1].data_ptr(), dys[2].data_ptr(), x.data_ptr(), dws[0].data_ptr(),
                                                  dws[1].data_ptr(), dws[2].data_ptr(), dt, N, C, H, W, K, ws.data_ptr(), nb, _st(x.device)), "tri_backward_filter")
    return dws


def _tri_bwd(dys, x, ws, K):
    """dx and the three weight gradients in ONE launch (slak_dwconv2d_tri_backward); None where there is no such launch"""
    L = _L(); lib = L.lib()
    N, C, H, W = x.shape
    dt = _dt(x.dtype)
    if not lib.slak_dwconv2d_tri_backward_supported(dt, N, C, H, W, K):
        return None
    nb = int(lib.slak_dwconv2d_tri_filter_workspace_bytes(dt, N, C, H, W, K))
    assert nb > 0
    wsb = torch.empty(nb, dtype=torch.uint8, device=x.device)
    dx = torch.full_like(x, float("nan"))
    dws = [torch.full((C, 1, kh, kw), float("nan"), dtype=torch.float32, device=x.device) for kh, kw in ((K, 5), (5, K), (5, 5))]
    L.check(lib.slak_dwconv2d_tri_backward(dys[0].data_ptr(), dys[1].data_ptr(), dys[2].data_ptr(), x.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(),
                                           ws[2].data_ptr(), dx.data_ptr(), dws[0].data_ptr(), dws[1].data_ptr(), dws[2].data_ptr(), dt, N, C, H, W, K,
                                           wsb.data_ptr(), nb, _st(x.device)), "tri_backward")
    return dx, dws
