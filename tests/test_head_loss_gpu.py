"""Pooled-LayerNorm head (slak_pool_ln_*, block_ops.pool_ln, SLaK.fused_head) and the cross-entropy criterion (slak_xent_*, slak_amd.loss)
on the GPU (pytest -m gpu).  The oracle is torch in float64 on the CPU on the same rounded inputs: F.layer_norm(x.mean([-2, -1])),
F.cross_entropy, and the two formulas of timm1/loss/cross_entropy.py:20-26 / :34-36 written out below.

Tolerances ("Parity"): a float32 result rtol 1e-4 / atol 1e-5; a bfloat16 / float16 result within one rounding of that
(2^-8 |ref| resp. 2^-11 |ref| on top of the float32 allowance); dweight / dbias 1e-4 of the largest entry, the way every weight gradient of the
block tail is checked (tests/test_block_tail_gpu.py).  Gradient entries of the criterion are as small as 1 / (N K): they are compared as
dlogits * count / g, the unnormalised p - t, with rtol 1e-4 / atol 1e-7.  A float16 gradient below 2^-14 is subnormal, where one rounding is
half the fixed spacing 2^-24 whatever the value: the rounding bound of a float16 entry is max(2^-11 |ref|, 2^-25).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
RND = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _sdt(dtype):
    from slak_amd import _lib
    return {torch.float32: _lib.SLAK_F32, torch.float16: _lib.SLAK_F16, torch.bfloat16: _lib.SLAK_BF16}[dtype]


def _check(got, ref, what, rnd=0.0, rtol=1e-4, atol=1e-5, floor=0.0):
    """|got - ref| <= max(rnd |ref|, floor) + rtol |ref| + atol, elementwise; ref float64 on the CPU"""
    got = got.detach().double().cpu()
    ref = ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what + ": not finite"
    tol = torch.clamp(rnd * ref.abs(), min=floor) + rtol * ref.abs() + atol
    over = (got - ref).abs() - tol
    i = int(over.argmax())
    assert over.max().item() <= 0, "%s: |%.9g - %.9g| = %.3e > %.3e at flat index %d" % (
        what, got.reshape(-1)[i], ref.reshape(-1)[i], (got - ref).abs().reshape(-1)[i], tol.reshape(-1)[i], i)


def _close_max(got, ref, rel, what):
    got, ref = got.detach().double().cpu(), ref.detach().double()
    err = (got - ref).abs().max().item()
    scale = max(1e-6, ref.abs().max().item())
    assert err <= rel * scale, "%s: err %.3e vs scale %.3e" % (what, err, scale)


# ================================================================ pool + LayerNorm
PL_SHAPES = [(2, 5, 1), (3, 7, 49), (2, 96, 49), (2, 768, 49), (2, 998, 49), (1, 1024, 144), (2, 1536, 36), (3, 64, 256)]
PL_HW = {1: (1, 1), 49: (7, 7), 144: (12, 12), 36: (6, 6), 256: (16, 16)}


def _pl_fwd(L, x, w, b, ydt, eps=1e-6):
    from slak_amd import _lib
    N, C, P = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
    y = torch.full((N, C), NAN, dtype=ydt, device=x.device)
    pooled = torch.full((N, C), NAN, device=x.device); mean = torch.full((N,), NAN, device=x.device); rstd = torch.full((N,), NAN, device=x.device)
    _lib.check(L.slak_pool_ln_forward(x.data_ptr(), _sdt(x.dtype), w.data_ptr(), b.data_ptr(), eps, y.data_ptr(), _sdt(ydt), pooled.data_ptr(),
                                      mean.data_ptr(), rstd.data_ptr(), N, C, P, _st(x.device)), "pool_ln fwd")
    return y, pooled, mean, rstd


def _pl_bwd(L, dy, pooled, w, mean, rstd, xshape, xdt):
    from slak_amd import _lib
    N, C, P = xshape[0], xshape[1], xshape[2] * xshape[3]
    dx = torch.full(xshape, NAN, dtype=xdt, device=dy.device)
    dw = torch.full((C,), NAN, device=dy.device); db = torch.full((C,), NAN, device=dy.device)
    nb = int(L.slak_pool_ln_workspace_bytes(N, C, P))
    ws = torch.empty(nb, dtype=torch.uint8, device=dy.device)
    _lib.check(L.slak_pool_ln_backward(dy.data_ptr(), _sdt(dy.dtype), pooled.data_ptr(), w.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                       _sdt(xdt), dw.data_ptr(), db.data_ptr(), N, C, P, ws.data_ptr(), nb, _st(dy.device)), "pool_ln bwd")
    return dx, dw, db


@pytest.mark.parametrize("xdt,ydt", [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32")])
@pytest.mark.parametrize("N,C,P", PL_SHAPES)
def test_pool_ln_matches_float64(N, C, P, xdt, ydt, gpu):
    """x = randn + 30: a one-pass variance of the pooled values loses about 3e-3 of it there, the two-pass one does not.  Through the C ABI
    and through block_ops.pool_ln (the same launches: the same bits)."""
    from slak_amd import _lib, block_ops
    L = _lib.lib()
    xdt, ydt = DT[xdt], DT[ydt]
    H, W = PL_HW[P]
    g = torch.Generator().manual_seed(1000 * C + P)
    x = (torch.randn(N, C, H, W, generator=g) + 30).to(xdt)
    w = torch.randn(C, generator=g) * 0.5 + 1
    b = torch.randn(C, generator=g) * 0.3
    dy = torch.randn(N, C, generator=g).to(ydt)
    xr = x.double().requires_grad_(True); wr = w.double().requires_grad_(True); br = b.double().requires_grad_(True)
    yr = F.layer_norm(xr.mean([-2, -1]), (C,), wr, br, 1e-6)
    yr.backward(dy.double())
    xg, wg, bg, dyg = x.to(gpu), w.to(gpu), b.to(gpu), dy.to(gpu)
    assert L.slak_pool_ln_supported(_sdt(xdt), N, C, P) == 1
    y, pooled, mean, rstd = _pl_fwd(L, xg, wg, bg, ydt)
    dx, dw, db = _pl_bwd(L, dyg, pooled, wg, mean, rstd, tuple(x.shape), xdt)
    _check(y, yr, "y", rnd=RND[ydt])
    _check(pooled, x.double().mean([-2, -1]), "pooled")
    _check(mean, x.double().mean([1, 2, 3]), "mean")
    _check(dx, xr.grad, "dx", rnd=RND[xdt])
    assert torch.equal(dx, dx[:, :, :1, :1].expand_as(dx)), "every pixel of a plane gets the same gradient"
    _close_max(dw, wr.grad, 1e-4, "dweight")
    _close_max(db, br.grad, 1e-4, "dbias")
    # a second run: the same bits
    y2, pooled2, mean2, rstd2 = _pl_fwd(L, xg, wg, bg, ydt)
    dx2, dw2, db2 = _pl_bwd(L, dyg, pooled2, wg, mean2, rstd2, tuple(x.shape), xdt)
    for a, c in ((y, y2), (pooled, pooled2), (mean, mean2), (rstd, rstd2), (dx, dx2), (dw, dw2), (db, db2)):
        assert torch.equal(a, c)
    # the autograd op: float32 for float32 x and under autocast, bfloat16 for bfloat16 x outside autocast
    hits = block_ops.head_hits
    xa = xg.clone().requires_grad_(True); wa = wg.clone().requires_grad_(True); ba = bg.clone().requires_grad_(True)
    if xdt == torch.bfloat16 and ydt == torch.float32:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ya = block_ops.pool_ln(xa, wa, ba, 1e-6)
    else:
        ya = block_ops.pool_ln(xa, wa, ba, 1e-6)
    assert ya.dtype == ydt and block_ops.head_hits == hits + 1
    ya.backward(dyg)
    assert torch.equal(ya, y) and torch.equal(xa.grad, dx) and torch.equal(wa.grad, dw) and torch.equal(ba.grad, db)


def test_pool_ln_autocast_of_float32_input_is_float32(gpu):
    from slak_amd import block_ops
    x = torch.randn(2, 16, 3, 3, device=gpu)
    w = torch.ones(16, device=gpu); b = torch.zeros(16, device=gpu)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = block_ops.pool_ln(x, w, b)
        want = F.layer_norm(x.mean([-2, -1]), (16,), w, b, 1e-6)
    assert y.dtype == want.dtype == torch.float32
    _check(y, F.layer_norm(x.double().cpu().mean([-2, -1]), (16,), eps=1e-6), "y")


# ================================================================ cross-entropy
XE_SHAPES = [(1, 2), (3, 10), (5, 63), (5, 64), (5, 65), (4, 1000), (2, 1001), (3, 4097), (2, 21841), (130, 1000)]
IGNORE = -100


def _xe_inputs(N, K, dtype, mode, seed):
    """logits * 30 (exp overflows without the row maximum); row 0: the label's logit 60 above the rest (loss near 0); row 1: all logits equal."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, K, generator=g) * 30
    y = torch.randint(0, K, (N,), generator=g)
    x[0, y[0]] = x[0].max() + 60
    if N > 1:
        x[1] = 7.0
    x = x.to(dtype)
    if mode == "soft":                                           # mixup's shape: two classes share 1 - eps, every class has the floor eps / K
        eps, lam = 0.1, 0.7
        y2 = y.flip(0)
        t = torch.full((N, K), eps / K)
        t[torch.arange(N), y] += (1 - eps) * lam
        t[torch.arange(N), y2] += (1 - eps) * (1 - lam)
        return x, t
    if mode == "ignore":
        y[N - 1] = IGNORE
    return x, y


def _xe_reference(x, target, mode, gout):
    """float64 on the CPU.  Returns loss, lse, count, dlogits (for the upstream gradient gout)."""
    xr = x.double().requires_grad_(True)
    lp = F.log_softmax(xr, -1)
    if mode == "soft":
        loss = torch.sum(-target.double() * lp, -1).mean()                                   # timm1/loss/cross_entropy.py:34-36
        count = float(x.shape[0])
    else:
        eps = 0.1 if mode in ("smooth", "ignore") else 0.0
        loss = F.cross_entropy(xr, target, label_smoothing=eps, ignore_index=IGNORE)
        count = float((target != IGNORE).sum())
        if mode == "smooth":                                                                 # timm1/loss/cross_entropy.py:20-26: the same number
            timm = (0.9 * -lp.gather(-1, target[:, None]).squeeze(1) + 0.1 * -lp.mean(-1)).mean()
            assert abs(float(timm.detach()) - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    (loss * gout).backward()
    return loss.detach(), torch.logsumexp(x.double(), -1), count, xr.grad


def _xe_fwd(L, x, target, eps, N, K):
    from slak_amd import _lib
    dev = x.device
    soft = target.is_floating_point()
    out = torch.full((2,), NAN, device=dev); lse = torch.full((N,), NAN, device=dev)
    nb = int(L.slak_xent_workspace_bytes(N, K))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.check(L.slak_xent_forward(x.data_ptr(), _sdt(x.dtype), x.stride(0), None if soft else target.data_ptr(), target.data_ptr() if soft else None,
                                   eps, IGNORE, out.data_ptr(), lse.data_ptr(), out.data_ptr() + 4, N, K, ws.data_ptr(), nb, _st(dev)), "xent fwd")
    return out, lse


def _xe_bwd(L, x, target, eps, out, lse, gout, N, K):
    from slak_amd import _lib
    soft = target.is_floating_point()
    d = torch.full((N, K), NAN, dtype=x.dtype, device=x.device)
    _lib.check(L.slak_xent_backward(x.data_ptr(), _sdt(x.dtype), x.stride(0), None if soft else target.data_ptr(), target.data_ptr() if soft else None,
                                    eps, IGNORE, lse.data_ptr(), out.data_ptr() + 4, gout.data_ptr(), d.data_ptr(), N, K, _st(x.device)), "xent bwd")
    return d


def _check_dlogits(d, ref, gout, count, dtype, what):
    """on the unnormalised scale p - t = dlogits * count / g: rtol 1e-4 / atol 1e-7, plus one rounding of the stored entry"""
    s = count / gout
    floor = 2.0 ** -25 * s if dtype == torch.float16 else 0.0
    _check(d.double().cpu() * s, ref * s, what, rnd=RND[dtype], rtol=1e-4, atol=1e-7, floor=floor)


@pytest.mark.parametrize("mode", ["hard", "smooth", "soft", "ignore"])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("N,K", XE_SHAPES)
def test_xent_matches_float64(N, K, dt, mode, gpu):
    from slak_amd import _lib, loss as LS
    L = _lib.lib()
    dtype = DT[dt]
    x, target = _xe_inputs(N, K, dtype, mode, seed=7 * K + N)
    eps = 0.0 if mode in ("hard", "soft") else 0.1
    xg, tg = x.to(gpu), target.to(gpu)
    assert L.slak_xent_supported(_sdt(dtype), N, K) == 1
    out, lse = _xe_fwd(L, xg, tg, eps, N, K)
    for gv in (1.0, 0.25):
        loss_r, lse_r, count, d_r = _xe_reference(x, target, mode, gv)
        assert float(out[1]) == count
        _check(lse, lse_r, "lse")
        if count == 0:                                           # every row ignored: 0 / 0, torch's 'mean' as well
            assert torch.isnan(out[0]) and torch.isnan(loss_r)
            d = _xe_bwd(L, xg, tg, eps, out, lse, torch.tensor([gv], device=gpu), N, K)
            assert torch.equal(d, torch.zeros_like(d))
            continue
        _check(out[0], loss_r, "loss")
        gout = torch.tensor([gv], device=gpu)                    # a device scalar, as autograd hands it over
        d = _xe_bwd(L, xg, tg, eps, out, lse, gout, N, K)
        _check_dlogits(d, d_r, gv, count, dtype, "dlogits (g = %g)" % gv)
        if mode == "ignore":
            assert torch.equal(d[N - 1], torch.zeros_like(d[N - 1])), "the ignored row's gradient is exactly zero"
            assert count == N - 1
        assert torch.equal(d, _xe_bwd(L, xg, tg, eps, out, lse, gout, N, K))
    out2, lse2 = _xe_fwd(L, xg, tg, eps, N, K)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(lse, lse2), "two runs: the same bits"
    # the Python op: one autograd node, float32 0-dim loss, the same launches
    hits = LS.fused_hits
    xa = xg.clone().requires_grad_(True)
    la = LS.cross_entropy(xa, tg, label_smoothing=eps, ignore_index=IGNORE)
    assert LS.fused_hits == hits + 1 and la.dtype == torch.float32 and la.dim() == 0
    if count > 0:
        assert torch.equal(la.detach(), out[0])
        (la * 0.25).backward()
        assert torch.equal(xa.grad, d)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_xent_unit_scale_logits(dt, gpu):
    """logits of unit scale, the head's at initialisation: the loss is ln K ~ 6.9 instead of ~100, so the same relative bound is 15 times tighter
    in absolute terms than on the scaled rows above"""
    from slak_amd import loss as LS
    N, K = 128, 1000
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(N, K, generator=g) * 0.5).to(DT[dt])
    y = torch.randint(0, K, (N,), generator=g)
    loss_r, _, count, d_r = _xe_reference(x, y, "smooth", 1.0)
    xa = x.to(gpu).requires_grad_(True)
    la = LS.cross_entropy(xa, y.to(gpu), label_smoothing=0.1)
    la.backward()
    _check(la, loss_r, "loss")
    _check_dlogits(xa.grad, d_r, 1.0, count, DT[dt], "dlogits")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_xent_noncontiguous_logits_view(dt, gpu):
    """rows of a wider matrix: the row stride travels to the kernel (rows start wherever the stride puts them), no copy"""
    from slak_amd import _lib, loss as LS
    L = _lib.lib()
    N, K = 6, 1001
    dtype = DT[dt]
    x, y = _xe_inputs(N, K, dtype, "smooth", seed=3)
    big = torch.full((N, K + 5), 1e4, dtype=dtype, device=gpu)
    big[:, 2:K + 2] = x.to(gpu)
    view = big[:, 2:K + 2]
    assert not view.is_contiguous()
    yg = y.to(gpu)
    out, lse = _xe_fwd(L, view, yg, 0.1, N, K)
    loss_r, lse_r, count, d_r = _xe_reference(x, y, "smooth", 1.0)
    _check(out[0], loss_r, "loss"); _check(lse, lse_r, "lse")
    d = _xe_bwd(L, view, yg, 0.1, out, lse, torch.ones(1, device=gpu), N, K)
    _check_dlogits(d, d_r, 1.0, count, dtype, "dlogits")
    va = view.detach().requires_grad_(True)
    la = LS.LabelSmoothingCrossEntropy(0.1)(va, yg)
    la.backward()
    assert torch.equal(la.detach(), out[0]) and torch.equal(va.grad, d)
    # a transposed view has no contiguous rows: the op copies it, the result is the formula's
    xt = x.to(gpu).t().contiguous().t()
    assert xt.stride(1) != 1
    _check(LS.LabelSmoothingCrossEntropy(0.1)(xt, yg), loss_r, "loss of a column-major view")


def test_criterion_classes_on_gpu(gpu):
    """the three classes main.py:398-403 picks from, bfloat16 logits as under autocast: float32 loss, fused path, gradient in the logits' dtype"""
    import slak_amd
    from slak_amd import loss as LS
    N, K = 8, 1000
    x, y = _xe_inputs(N, K, torch.bfloat16, "hard", seed=11)
    _, t = _xe_inputs(N, K, torch.bfloat16, "soft", seed=11)
    for crit, target, mode in ((slak_amd.CrossEntropyLoss(), y, "hard"), (slak_amd.CrossEntropyLoss(label_smoothing=0.1), y, "smooth"),
                               (slak_amd.LabelSmoothingCrossEntropy(0.1), y, "smooth"), (slak_amd.SoftTargetCrossEntropy(), t, "soft")):
        hits = LS.fused_hits
        xa = x.to(gpu).requires_grad_(True)
        la = crit(xa, target.to(gpu))
        assert LS.fused_hits == hits + 1 and la.dtype == torch.float32
        la.backward()
        loss_r, _, count, d_r = _xe_reference(x, target, mode, 1.0)
        _check(la, loss_r, "loss")
        assert xa.grad.dtype == torch.bfloat16
        _check_dlogits(xa.grad, d_r, 1.0, count, torch.bfloat16, "dlogits")
    # arguments the kernel does not take run torch's formula, never another result
    hits = LS.fused_hits
    xf = x.float().to(gpu)
    got = LS.cross_entropy(xf, t.to(gpu), label_smoothing=0.2)
    _check(got, F.cross_entropy(x.double(), t.double(), label_smoothing=0.2), "soft targets with label smoothing")
    w = torch.rand(K, device=gpu)
    assert torch.equal(slak_amd.CrossEntropyLoss(weight=w)(xf, y.to(gpu)), F.cross_entropy(xf, y.to(gpu), weight=w))
    assert LS.fused_hits == hits


# ================================================================ model and loop
def _small_model(gpu, seed=0):
    import slak_amd.slak_model as M
    torch.manual_seed(seed)
    return M.SLaK(in_chans=3, num_classes=10, depths=(1, 1, 1, 1), dims=(8, 16, 32, 64), drop_path_rate=0.0, kernel_size=(7, 7, 7, 7, 5),
                  Decom=True).to(gpu)


def _run(net, xs, ys, autocast):
    for p in net.parameters():
        p.grad = None
    if autocast:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = net(xs)
            loss = F.cross_entropy(logits.float(), ys)
    else:
        logits = net(xs)
        loss = F.cross_entropy(logits, ys)
    loss.backward()
    return logits.detach().clone(), {n: p.grad.detach().clone() for n, p in net.named_parameters()}


def test_model_fused_head_matches_the_torch_ops(gpu):
    from slak_amd import block_ops
    net = _small_model(gpu)
    g = torch.Generator(device=gpu).manual_seed(4)
    xs = torch.randn(3, 3, 64, 64, device=gpu, generator=g); ys = torch.randint(0, 10, (3,), device=gpu, generator=g)
    assert net.fused_head is False
    hits = block_ops.head_hits
    l0, g0 = _run(net, xs, ys, False)
    l0a, _ = _run(net, xs, ys, True)
    assert block_ops.head_hits == hits                          # flag off: the two torch ops
    net.fused_head = True
    l1, g1 = _run(net, xs, ys, False)
    assert block_ops.head_hits == hits + 1
    l1a, _ = _run(net, xs, ys, True)
    assert block_ops.head_hits == hits + 2 and l1.dtype == l0.dtype and l1a.dtype == l0a.dtype
    _check(l1, l0.double().cpu(), "logits")
    for n in g0:
        _check(g1[n], g0[n].double().cpu(), "gradient of " + n)
    _close_max(l1a, l0a.double().cpu(), 1e-2, "logits under bfloat16 autocast")
    # a forward hook on the final norm: the module is called (the hook fires), the fused op is not
    seen = []
    h = net.norm.register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
    try:
        hits = block_ops.head_hits
        l2, _ = _run(net, xs, ys, False)
        assert seen == [(3, 64)] and block_ops.head_hits == hits
        assert torch.equal(l2, l0)
    finally:
        h.remove()


def _loop(net0, crit, targets, xs, gpu):
    """four optimizer steps, two micro-batches each, loss / 2 (the update_freq form of engine.py:79-81)"""
    import copy
    net = copy.deepcopy(net0)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0.05)
    losses = []
    for step in range(4):
        for mb in range(2):
            i = (2 * step + mb) % len(xs)
            loss = crit(net(xs[i]), targets[i])
            losses.append(float(loss.detach()))
            (loss / 2).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    return losses


@pytest.mark.parametrize("kind", ["label_smoothing", "soft_target"])
def test_training_loop_matches_the_torch_formula(kind, gpu):
    import slak_amd
    from slak_amd import loss as LS
    net0 = _small_model(gpu, seed=2)
    g = torch.Generator(device=gpu).manual_seed(9)
    xs = [torch.randn(3, 3, 64, 64, device=gpu, generator=g) for _ in range(4)]
    ys = [torch.randint(0, 10, (3,), device=gpu, generator=g) for _ in range(4)]
    if kind == "label_smoothing":
        crit = slak_amd.LabelSmoothingCrossEntropy(0.1)
        targets = ys

        def formula(x, y):                                       # timm1/loss/cross_entropy.py:20-26 in float32 torch ops
            lp = F.log_softmax(x.float(), -1)
            return (0.9 * -lp.gather(-1, y[:, None]).squeeze(1) + 0.1 * -lp.mean(-1)).mean()
    else:
        crit = slak_amd.SoftTargetCrossEntropy()
        targets = []
        for y in ys:
            t = torch.full((3, 10), 0.01, device=gpu)
            t[torch.arange(3), y] += 0.9 * 0.7
            t[torch.arange(3), y.flip(0)] += 0.9 * 0.3
            targets.append(t)

        def formula(x, t):                                       # timm1/loss/cross_entropy.py:34-36
            return torch.sum(-t * F.log_softmax(x.float(), -1), -1).mean()
    hits = LS.fused_hits
    got = _loop(net0, crit, targets, xs, gpu)
    assert LS.fused_hits == hits + 8
    want = _loop(net0, formula, targets, xs, gpu)
    assert LS.fused_hits == hits + 8
    assert len(got) == 8
    np.testing.assert_allclose(got, want, rtol=2e-4, atol=0)
