"""Pooled-LayerNorm head and cross-entropy criterion -- the host-side part: the `*_supported` / `*_workspace_bytes` queries, the argument
validation of the entry points (status codes before anything touches a GPU), the criterion classes on CPU tensors against their formulas in
float64 (timm1/loss/cross_entropy.py:20-26, :34-36; F.cross_entropy), and the model flag's default."""
import ctypes

import pytest
import torch
import torch.nn.functional as F


@pytest.fixture(scope="module")
def L():
    from slak_amd import build, _lib
    build.build()
    return _lib.lib()


def _p():
    buf = ctypes.create_string_buffer(64)                    # never dereferenced: the argument checks come first
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_queries_answer_without_a_device(L):
    from slak_amd import _lib
    F32, F16, BF16 = _lib.SLAK_F32, _lib.SLAK_F16, _lib.SLAK_BF16
    for dt, N, C, P, want in ((F32, 128, 768, 49, 1), (BF16, 128, 998, 49, 1), (F32, 1, 2048, 1024, 1), (BF16, 2, 5, 1, 1), (F16, 2, 96, 49, 0),
                              (F32, 2, 2049, 49, 0), (F32, 2, 96, 1025, 0), (F32, 0, 96, 49, 0), (F32, 2, 0, 49, 0), (F32, 2048, 2048, 1024, 0), (7, 2, 96, 49, 0)):
        assert L.slak_pool_ln_supported(dt, N, C, P) == want, (dt, N, C, P)
    assert L.slak_pool_ln_workspace_bytes(128, 768, 49) >= 128 * 2 * 768 * 4
    assert L.slak_pool_ln_workspace_bytes(0, 768, 49) == 0
    for dt, N, K, want in ((F32, 128, 1000, 1), (BF16, 2, 21841, 1), (F16, 1, 1, 1), (F32, 3, 32768, 1), (F32, 3, 32769, 0), (F32, 0, 10, 0),
                           (F32, 3, 0, 0), (9, 3, 10, 0)):
        assert L.slak_xent_supported(dt, N, K) == want, (dt, N, K)
    assert L.slak_xent_workspace_bytes(128, 1000) >= 2 * 128 * 4
    assert L.slak_xent_workspace_bytes(128, 0) == 0


def test_pool_ln_entry_points_validate_on_the_host(L):
    from slak_amd import _lib
    keep, p = _p()
    F32 = _lib.SLAK_F32
    fwd = lambda x, N, C, P, xdt=F32, ydt=F32: L.slak_pool_ln_forward(x, xdt, p, p, 1e-6, p, ydt, p, p, p, N, C, P, None)
    bwd = lambda dy, N, C, P, ws=p, nb=1 << 30: L.slak_pool_ln_backward(dy, F32, p, p, p, p, p, F32, p, p, N, C, P, ws, nb, None)
    assert fwd(None, 2, 96, 49) == _lib.ERR_INVALID_ARG and bwd(None, 2, 96, 49) == _lib.ERR_INVALID_ARG
    for N, C, P in ((0, 96, 49), (-1, 96, 49), (2, 0, 49), (2, 96, 0)):
        assert fwd(p, N, C, P) == _lib.ERR_INVALID_ARG and bwd(p, N, C, P) == _lib.ERR_INVALID_ARG
    assert fwd(p, 2, 96, 49, xdt=11) == _lib.ERR_INVALID_ARG
    for N, C, P in ((2, 2049, 49), (2, 96, 1025), (4096, 2048, 1024)):
        assert fwd(p, N, C, P) == _lib.ERR_UNSUPPORTED and bwd(p, N, C, P) == _lib.ERR_UNSUPPORTED
    assert fwd(p, 2, 96, 49, xdt=_lib.SLAK_F16) == _lib.ERR_UNSUPPORTED and fwd(p, 2, 96, 49, ydt=_lib.SLAK_F16) == _lib.ERR_UNSUPPORTED
    assert bwd(p, 2, 96, 49, ws=None, nb=0) == 3 and bwd(p, 2, 96, 49, nb=16) == 3              # SLAK_ERR_WORKSPACE


def test_xent_entry_points_validate_on_the_host(L):
    from slak_amd import _lib
    keep, p = _p()
    F32 = _lib.SLAK_F32
    fwd = lambda x, lab, soft, N, K, dt=F32, eps=0.1, ws=p, nb=1 << 30: L.slak_xent_forward(x, dt, K, lab, soft, eps, -100, p, p, p, N, K, ws, nb, None)
    bwd = lambda x, lab, soft, N, K, dt=F32, eps=0.1: L.slak_xent_backward(x, dt, K, lab, soft, eps, -100, p, p, p, p, N, K, None)
    for f in (fwd, bwd):
        assert f(None, p, None, 4, 10) == _lib.ERR_INVALID_ARG
        assert f(p, p, p, 4, 10) == _lib.ERR_INVALID_ARG                  # both targets
        assert f(p, None, None, 4, 10) == _lib.ERR_INVALID_ARG            # neither
        assert f(p, p, None, 0, 10) == _lib.ERR_INVALID_ARG and f(p, p, None, -3, 10) == _lib.ERR_INVALID_ARG
        assert f(p, p, None, 4, 0) == _lib.ERR_INVALID_ARG and f(p, None, p, 4, -1) == _lib.ERR_INVALID_ARG
        assert f(p, p, None, 4, 10, dt=5) == _lib.ERR_INVALID_ARG
        assert f(p, p, None, 4, 10, eps=1.0) == _lib.ERR_INVALID_ARG and f(p, p, None, 4, 10, eps=-0.1) == _lib.ERR_INVALID_ARG
        assert f(p, p, None, 4, 32769) == _lib.ERR_UNSUPPORTED and f(p, None, p, 1, 40000, dt=_lib.SLAK_BF16) == _lib.ERR_UNSUPPORTED
    assert L.slak_xent_forward(p, F32, 9, p, None, 0.0, -100, p, p, p, 4, 10, p, 1 << 30, None) == _lib.ERR_INVALID_ARG   # row stride < K
    assert fwd(p, p, None, 4, 10, ws=None, nb=0) == 3 and fwd(p, p, None, 4, 10, nb=8) == 3            # SLAK_ERR_WORKSPACE
    assert L.slak_xent_forward(p, F32, 10, p, None, 0.0, -100, None, p, p, 4, 10, p, 1 << 30, None) == _lib.ERR_INVALID_ARG
    assert L.slak_xent_backward(p, F32, 10, p, None, 0.0, -100, p, p, None, p, 4, 10, None) == _lib.ERR_INVALID_ARG        # grad_out is a pointer


def _cases():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 11, generator=g) * 4
    y = torch.randint(0, 11, (6,), generator=g)
    t = torch.rand(6, 11, generator=g)
    t = t / t.sum(-1, keepdim=True)
    return x, y, t


def test_criteria_on_cpu_equal_their_float64_formulas():
    import slak_amd
    from slak_amd import loss
    x, y, t = _cases()
    xd, td = x.double(), t.double()
    lp = F.log_softmax(xd, -1)
    before = loss.fused_hits
    # torch.nn.CrossEntropyLoss (main.py:403), with smoothing and an ignored row as well
    assert torch.allclose(slak_amd.CrossEntropyLoss()(x, y).double(), F.cross_entropy(xd, y), rtol=1e-4, atol=1e-5)
    y2 = y.clone(); y2[2] = -100
    got = slak_amd.CrossEntropyLoss(label_smoothing=0.1)(x, y2)
    assert got.dtype == torch.float32 and got.dim() == 0
    assert torch.allclose(got.double(), F.cross_entropy(xd, y2, label_smoothing=0.1), rtol=1e-4, atol=1e-5)
    w = torch.rand(11)
    assert torch.allclose(slak_amd.CrossEntropyLoss(weight=w, reduction="sum")(x, y), F.cross_entropy(x, y, weight=w, reduction="sum"))
    assert isinstance(slak_amd.CrossEntropyLoss(), torch.nn.CrossEntropyLoss)
    # timm1/loss/cross_entropy.py:20-26
    want = (0.9 * -lp.gather(-1, y[:, None]).squeeze(1) + 0.1 * -lp.mean(-1)).mean()
    crit = slak_amd.LabelSmoothingCrossEntropy(0.1)
    assert crit.smoothing == 0.1 and crit.confidence == 0.9
    assert torch.allclose(crit(x, y).double(), want, rtol=1e-4, atol=1e-5)
    assert torch.allclose(slak_amd.LabelSmoothingCrossEntropy()(x, y).double(), want, rtol=1e-4, atol=1e-5)      # smoothing defaults to 0.1
    # timm1/loss/cross_entropy.py:34-36
    want = torch.sum(-td * lp, -1).mean()
    assert torch.allclose(slak_amd.SoftTargetCrossEntropy()(x, t).double(), want, rtol=1e-4, atol=1e-5)
    assert torch.allclose(loss.cross_entropy(x, t, label_smoothing=0.2).double(), F.cross_entropy(xd, td, label_smoothing=0.2), rtol=1e-4, atol=1e-5)
    assert loss.fused_hits == before                          # CPU tensors never count as served by the kernel
    # gradients flow through the torch formula
    xg = x.clone().requires_grad_(True)
    (slak_amd.LabelSmoothingCrossEntropy(0.1)(xg, y) / 2).backward()
    xr = xd.clone().requires_grad_(True)
    ((0.9 * -F.log_softmax(xr, -1).gather(-1, y[:, None]).squeeze(1) + 0.1 * -F.log_softmax(xr, -1).mean(-1)).mean() / 2).backward()
    assert torch.allclose(xg.grad.double() * 12, xr.grad * 12, rtol=1e-4, atol=1e-6)


def test_package_exports_the_three_criteria():
    import slak_amd
    for n in ("CrossEntropyLoss", "LabelSmoothingCrossEntropy", "SoftTargetCrossEntropy"):
        assert n in slak_amd.__all__ and isinstance(getattr(slak_amd, n), type)


def test_fused_head_is_off_by_default():
    from slak_amd import slak_model
    assert slak_model.SLaK.fused_head is False
    m = slak_model.SLaK(num_classes=5, depths=(1, 1, 1, 1), dims=(8, 16, 32, 64), kernel_size=(7, 7, 7, 7, 5), Decom=True)
    assert m.fused_head is False
