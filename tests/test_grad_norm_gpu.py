"""GPU tests of the fused gradient norm / clipping / loss-scale handling of MaskedAdamW (pytest -m gpu):
``MaskedAdamW.step_with_grad_norm``, ``slak_amd.scaler.NativeScalerWithGradNormCount``, ``Masking.step(clip_grad=...)``.

Shapes: the ragged set of test_optim_ema_gpu.test_masked_adamw_matches_torch_adamw (crosses the 4096-element chunk by one, tensors smaller
than a wave) plus a zero-element tensor.  Every bound below is derived where it is used; none is measured.
"""
import contextlib
import io
import math
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
sys.path.insert(0, GOLDEN)

SHAPES = [(96, 1, 51, 5), (384, 96), (96,), (5,), (1,), (33, 7, 3), (4097,), (70001,), (0,)]
NO_GRAD = 3                      # index of the parameter whose grad is None


def _params(base, dev):
    return [torch.nn.Parameter(t.clone().to(dev)) for t in base]


def _base(seed):
    gen = torch.Generator().manual_seed(seed)
    return gen, [torch.randn(s, generator=gen) * 0.05 for s in SHAPES]


def _unaligned_views(tensors, dev):
    """Views of ONE flat fp32 buffer, each starting at an element offset that is no multiple of 4 (so no view is 16-byte aligned: the
    scalar path), as DDP bucket views may."""
    offs, at = [], 1
    for t in tensors:
        offs.append(at)
        at += t.numel()
        if at % 4 == 0:
            at += 1
    flat = torch.zeros(at + 3, dtype=torch.float32, device=dev)
    views = []
    for t, o in zip(tensors, offs):
        v = flat[o:o + t.numel()].view(t.shape)
        v.copy_(t)
        assert t.numel() == 0 or v.data_ptr() % 16 != 0
        views.append(v)
    return flat, views


def _norm64(grads, inv_scale):
    """float32(sqrt(sum in fp64 of (g * inv_scale rounded to fp32)^2)) on the CPU."""
    total = 0.0
    for g in grads:
        if g is None:
            continue
        u = (g.detach().cpu().numpy().astype(np.float32) * np.float32(inv_scale)).astype(np.float32).astype(np.float64)
        total += float(np.sum(u * u))
    return np.float32(math.sqrt(total))


def _within_ulps(got, want, ulps):
    got, want = np.float32(got), np.float32(want)
    return abs(float(got) - float(want)) <= ulps * float(np.spacing(want))


@pytest.fixture(scope="module")
def ragged_grads():
    gen = torch.Generator().manual_seed(11)
    return [torch.randn(s, generator=gen) * 0.1 for s in SHAPES]


# ------------------------------------------------------------------ 1. the norm
@pytest.mark.parametrize("inv_scale", [1.0, 2.0 ** -16])
def test_norm_unaligned_views_within_one_ulp(inv_scale, ragged_grads, gpu):
    """Bound: the squares are exact in fp64 (24-bit x 24-bit significands), an fp64 sum of < 2^17 terms errs far below 2^-30 relative,
    so only the final rounding of sqrt(total) to fp32 counts: 1 ulp.  Reproducible: two calls give the same bits."""
    from slak_amd.optim_factory import MaskedAdamW
    _, base = _base(0)
    ps = _params(base, gpu)
    opt = MaskedAdamW(ps, lr=1e-3)
    _, views = _unaligned_views(ragged_grads, gpu)
    for i, (p, v) in enumerate(zip(ps, views)):
        p.grad = None if i == NO_GRAD else v
    inv = None if inv_scale == 1.0 else torch.tensor(inv_scale, device=gpu)
    n1 = opt.step_with_grad_norm(inv_scale=inv)
    c1 = opt.last_grad_control.clone()
    n2 = opt.step_with_grad_norm(inv_scale=inv)
    c2 = opt.last_grad_control.clone()
    assert n1.shape == () and n1.dtype == torch.float32 and n1.is_cuda
    want = _norm64([p.grad for p in ps], inv_scale)
    got = float(n1)
    print("norm", got, "fp64", float(want), "ulp", float(np.spacing(want)))
    assert _within_ulps(got, want, 1)
    assert torch.equal(n1, n2) and torch.equal(c1, c2)
    assert c1.tolist() == [inv_scale, 1.0, 0.0, got]
    assert torch.equal(ps[NO_GRAD].detach().cpu(), base[NO_GRAD])               # no gradient: untouched


# ------------------------------------------------------------------ 2. more than one plan
def test_norm_spans_plans(gpu):
    """70 parameter groups > SLAK_ADAMW_MAX_GROUPS = 64: two plans, one norm over both, and both plans step exactly as step() does."""
    from slak_amd.optim_factory import MaskedAdamW
    gen = torch.Generator().manual_seed(3)
    base = [torch.randn(5000 if i == 67 else i + 1, generator=gen) * 0.05 for i in range(70)]
    grads = [(torch.randn(t.shape, generator=gen) * 0.1).to(gpu) for t in base]
    pa, pb = _params(base, gpu), _params(base, gpu)
    oa = MaskedAdamW([dict(params=[p], lr=1e-3 * (1 + i % 5)) for i, p in enumerate(pa)])
    ob = MaskedAdamW([dict(params=[p], lr=1e-3 * (1 + i % 5)) for i, p in enumerate(pb)])
    for a, b, g in zip(pa, pb, grads):
        a.grad, b.grad = g.clone(), g.clone()
    norm = oa.step_with_grad_norm()
    assert len(oa._plans) == 2
    want = _norm64(grads, 1.0)
    print("norm", float(norm), "fp64", float(want))
    assert _within_ulps(float(norm), want, 1)
    ob.step()
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
    assert not torch.equal(pa[69].detach().cpu(), base[69])


# ------------------------------------------------------------------ 3. the clip coefficient
def test_clip_coefficient(ragged_grads, gpu):
    """Below the norm: within 2 fp32 ulp of clip / (norm + 1e-6) evaluated in fp64 from the returned norm (one rounding for the sum,
    one for the division).  Above the norm, and without clipping: exactly 1."""
    from slak_amd.optim_factory import MaskedAdamW
    _, base = _base(0)
    ps = _params(base, gpu)
    opt = MaskedAdamW(ps, lr=0.0, weight_decay=0.0)
    for p, g in zip(ps, ragged_grads):
        p.grad = g.to(gpu)
    norm = float(opt.step_with_grad_norm())
    assert opt.last_grad_control[1].item() == 1.0
    for clip in (0.5 * norm, 0.999 * norm, 0.01):
        n = float(opt.step_with_grad_norm(clip_grad=clip))
        want = clip / (float(np.float32(n)) + 1e-6)
        got = opt.last_grad_control[1].item()
        print("clip", clip, "coef", got, "fp64", want)
        assert n == norm and got < 1.0 and _within_ulps(got, np.float32(want), 2)
    for clip in (2.0 * norm, 1.01 * norm, 1e6):
        assert float(opt.step_with_grad_norm(clip_grad=clip)) == norm
        assert opt.last_grad_control[1].item() == 1.0


# ------------------------------------------------------------------ 4. the update, bit for bit against step()
def test_update_equals_step_on_prescaled_gradients(ragged_grads, gpu):
    """The twin gets g * ctl[0], then * ctl[1] (two fp32 torch multiplies: what unscale_ and clip_grad_norm_ leave in the tensor) and
    takes the existing step(): everything is torch.equal over 4 steps with a changing lr, masks and the bf16 cache on, and the gradients
    handed to the fused call are not modified."""
    from slak_amd import block_ops
    from slak_amd.optim_factory import MaskedAdamW
    gen, base = _base(1)
    pa, pb = _params(base, gpu), _params(base, gpu)
    mk = {i: (torch.rand(base[i].shape, generator=gen) < 0.6).float().to(gpu) for i in (0, 1, 7)}
    old = block_ops.cache_lowp_weights
    block_ops.cache_lowp_weights = True
    try:
        ca, cb = block_ops.lowp_param(pa[1]), block_ops.lowp_param(pb[1])

        def groups(ps):
            return [dict(params=ps[:2], lr=4e-3, weight_decay=0.05), dict(params=ps[2:5], lr=1e-3, weight_decay=0.0, betas=(0.8, 0.99)),
                    dict(params=ps[5:], lr=2e-3, weight_decay=0.3, eps=1e-6)]
        oa, ob = MaskedAdamW(groups(pa), lr=1e-3), MaskedAdamW(groups(pb), lr=1e-3)
        oa.set_masks({pa[i]: m for i, m in mk.items()})
        ob.set_masks({pb[i]: m for i, m in mk.items()})
        inv = torch.tensor(2.0 ** -10, device=gpu)
        for step in range(4):
            gs = [(torch.randn(s, generator=gen) * 0.1 * 1024.0) for s in SHAPES]
            _, views = _unaligned_views(gs, gpu)
            keep = [v.clone() for v in views]
            for i, (a, v) in enumerate(zip(pa, views)):
                a.grad = None if i == NO_GRAD else v
            for o in (oa, ob):
                for g in o.param_groups:
                    g["lr"] = g["lr"] * 0.9
            clip = (0.5, None, 1e9, 2.0)[step]                           # clipping, none, far above the norm, clipping
            oa.step_with_grad_norm(clip_grad=clip, inv_scale=inv)
            ctl = oa.last_grad_control
            assert ctl[0].item() == 2.0 ** -10 and ctl[2].item() == 0.0 and (ctl[1].item() < 1.0) == (clip in (0.5, 2.0))
            for i, (b, v) in enumerate(zip(pb, keep)):
                b.grad = None if i == NO_GRAD else (v * ctl[0]) * ctl[1]
            ob.step()
            for v, k in zip(views, keep):
                assert torch.equal(v, k)                                  # read only
            for i, (a, b) in enumerate(zip(pa, pb)):
                assert torch.equal(a.detach(), b.detach()), (step, i)
                if i != NO_GRAD:
                    for k in ("exp_avg", "exp_avg_sq", "step"):
                        assert torch.equal(oa.state[a][k], ob.state[b][k]), (step, i, k)
            for i, m in mk.items():
                assert bool((pa[i].detach()[m == 0] == 0).all())
            assert block_ops.lowp_param(pa[1]) is ca and torch.equal(ca, cb) and torch.equal(ca, pa[1].detach().to(torch.bfloat16))
        assert float(oa.state[pa[0]]["step"]) == 4.0
    finally:
        block_ops.cache_lowp_weights = old
        block_ops._lowp_cache.clear()


# ------------------------------------------------------------------ 5. against torch's own sequence
def test_against_unscale_clip_adamw(gpu):
    """GradScaler.unscale_ (g *= inv_scale), clip_grad_norm_, torch.optim.AdamW(foreach=False).  Tolerance: 3e-6 of each tensor's max
    magnitude, that of test_masked_adamw_matches_torch_adamw and for its reason (torch's foreach / fused / CPU AdamW differ among
    themselves at the 1e-7 level per step; errors accumulate through exp_avg)."""
    from slak_amd.optim_factory import MaskedAdamW
    gen, base = _base(2)
    pa, pb = _params(base, gpu), _params(base, gpu)

    def groups(ps):
        return [dict(params=ps[:2], lr=4e-3, weight_decay=0.05), dict(params=ps[2:5], lr=1e-3, weight_decay=0.0, betas=(0.8, 0.99)),
                dict(params=ps[5:], lr=2e-3, weight_decay=0.3, eps=1e-6)]
    ours, ref = MaskedAdamW(groups(pa), lr=1e-3), torch.optim.AdamW(groups(pb), lr=1e-3, foreach=False)
    inv = torch.tensor(2.0 ** -16, device=gpu)
    for step in range(4):
        for i, (a, b) in enumerate(zip(pa, pb)):
            if i == NO_GRAD:
                continue
            gr = (torch.randn(a.shape, generator=gen) * 0.1 * 65536.0).to(gpu)
            a.grad, b.grad = gr.clone(), gr * inv
        for o in (ours, ref):
            for g in o.param_groups:
                g["lr"] = g["lr"] * 0.9
        clip = 1.0 if step % 2 == 0 else 1e9
        norm = ours.step_with_grad_norm(clip_grad=clip, inv_scale=inv)
        want = torch.nn.utils.clip_grad_norm_(pb, clip)
        ref.step()
        assert abs(float(norm) - float(want)) <= 3e-6 * float(want)
        for i, (a, b) in enumerate(zip(pa, pb)):
            tol = 3e-6 * float(b.detach().abs().max()) + 1e-12 if b.numel() else 0.0
            assert b.numel() == 0 or float((a.detach() - b.detach()).abs().max()) <= tol, (step, i)


# ------------------------------------------------------------------ 6. overflow
def test_overflow_skips_the_step_and_backs_the_scale_off(gpu):
    """6 updates with growth_interval=2; an inf in the last element of the last non-empty tensor on update 2, a NaN in the one-element
    tensor on update 4 (data, not a fault).  On those: nothing changes, the norm is non-finite, found_inf is 1.  The scale and growth
    tracker follow, exactly, a torch.cuda.amp.GradScaler driving torch.optim.AdamW on the same gradients."""
    from slak_amd.optim_factory import MaskedAdamW
    from slak_amd.scaler import NativeScalerWithGradNormCount
    gen, base = _base(4)
    pa, pb = _params(base, gpu), _params(base, gpu)
    oa, ob = MaskedAdamW(pa, lr=1e-2), torch.optim.AdamW(pb, lr=1e-2, foreach=False)
    ours = NativeScalerWithGradNormCount(growth_interval=2)
    ref = torch.cuda.amp.GradScaler(growth_interval=2)
    last = max(i for i, s in enumerate(SHAPES) if int(np.prod(s)) > 0)
    one = SHAPES.index((1,))
    scales = []
    for update in range(1, 7):
        G = [(torch.randn(s, generator=gen) * 1e-3).to(gpu) for s in SHAPES]
        if update == 2:
            G[last].view(-1)[-1] = float("inf")
        if update == 4:
            G[one].view(-1)[0] = float("nan")
        bad = update in (2, 4)
        before = [p.detach().clone() for p in pa]
        state = {i: {k: v.clone() for k, v in oa.state[p].items()} for i, p in enumerate(pa) if p in oa.state and oa.state[p]}
        for p in pa + pb:
            p.grad = None
        norm = ours(sum((p * g).sum() for p, g in zip(pa, G)), oa, clip_grad=1.0, parameters=pa)
        ref.scale(sum((p * g).sum() for p, g in zip(pb, G))).backward()
        for a, b in zip(pa, pb):
            assert torch.equal(a.grad, b.grad) or bad                      # the same (scaled) gradients
        ref.unscale_(ob)
        ref.step(ob)
        ref.update()
        ctl = oa.last_grad_control
        assert ctl[2].item() == (1.0 if bad else 0.0)
        assert math.isfinite(float(norm)) != bad
        if bad:
            for i, (p, w) in enumerate(zip(pa, before)):
                assert torch.equal(p.detach(), w), (update, i)
                for k, v in state.get(i, {}).items():
                    assert torch.equal(oa.state[p][k], v), (update, i, k)
        assert torch.equal(ours._scaler._scale, ref._scale) and torch.equal(ours._scaler._growth_tracker, ref._growth_tracker), update
        scales.append((float(ref._scale), int(ref._growth_tracker)))
    assert scales == [(65536.0, 1), (32768.0, 0), (32768.0, 1), (16384.0, 0), (16384.0, 1), (32768.0, 0)]
    assert float(oa.state[pa[0]]["step"]) == 4.0 == float(ob.state[pb[0]]["step"])
    for a, b in zip(pa, pb):                                               # and the four clean updates were AdamW's (clip far above the norm)
        assert b.numel() == 0 or float((a.detach() - b.detach()).abs().max()) <= 3e-6 * float(b.detach().abs().max()) + 1e-12


# ------------------------------------------------------------------ 7. the mirror class
def test_mirror_class_surface(gpu):
    from slak_amd.optim_factory import MaskedAdamW
    from slak_amd.scaler import NativeScalerWithGradNormCount
    assert NativeScalerWithGradNormCount.state_dict_key == "amp_scaler"
    fresh = torch.cuda.amp.GradScaler().state_dict()
    ours = NativeScalerWithGradNormCount()
    assert ours.state_dict() == fresh and list(ours.state_dict()) == list(fresh) and fresh["scale"] == 65536.0
    # a GradScaler that has backed off once
    p = torch.nn.Parameter(torch.ones(4, device=gpu))
    sgd = torch.optim.SGD([p], lr=0.1)
    ref = torch.cuda.amp.GradScaler()
    ref.scale((p * torch.tensor([1.0, float("inf"), 1.0, 1.0], device=gpu)).sum()).backward()
    ref.step(sgd)
    ref.update()
    assert ref.state_dict()["scale"] == 32768.0
    ours.load_state_dict(ref.state_dict())
    assert ours.state_dict() == ref.state_dict()
    # update_grad=False: backward only
    _, base = _base(5)
    ps = _params(base, gpu)
    opt = MaskedAdamW(ps, lr=1e-2)
    G = [torch.full(s, 0.5, device=gpu) for s in SHAPES]
    assert ours(sum((q * g).sum() for q, g in zip(ps, G)), opt, update_grad=False) is None
    assert all(torch.equal(q.detach().cpu(), b) for q, b in zip(ps, base))
    assert torch.equal(ps[0].grad, G[0] * 32768.0) and float(ours._scaler._scale) == 32768.0   # the loaded scale, on the device
    for q in ps:
        q.grad = None
    norm = ours(sum((q * g).sum() for q, g in zip(ps, G)), opt, clip_grad=None)
    assert _within_ulps(float(norm), _norm64(G, 1.0), 1) and not torch.equal(ps[0].detach().cpu(), base[0])
    assert torch.equal(ps[0].grad, G[0] * 32768.0)                                          # the documented difference: still scaled
    # enabled=False (bf16): scale 1, never updated; norm, clipping and step still happen
    off = NativeScalerWithGradNormCount(enabled=False)
    ps = _params(base, gpu)
    opt = MaskedAdamW(ps, lr=1e-2)
    norm = off(sum((q * g).sum() for q, g in zip(ps, G)), opt, clip_grad=1.0)
    assert off._scaler.get_scale() == 1.0 and off.state_dict() == torch.cuda.amp.GradScaler(enabled=False).state_dict()
    assert torch.equal(ps[0].grad, G[0]) and opt.last_grad_control[0].item() == 1.0 and opt.last_grad_control[1].item() < 1.0
    assert _within_ulps(float(norm), _norm64(G, 1.0), 1) and not torch.equal(ps[0].detach().cpu(), base[0])
    # any other optimizer: the reference's own sequence
    q = torch.nn.Parameter(torch.ones(5, device=gpu))
    sgd = torch.optim.SGD([q], lr=0.5)
    fb = NativeScalerWithGradNormCount()
    norm = fb((q * torch.arange(5.0, device=gpu)).sum(), sgd, clip_grad=None, parameters=[q])
    assert abs(float(norm) - math.sqrt(30.0)) < 1e-5
    assert torch.equal(q.detach(), 1.0 - 0.5 * torch.arange(5.0, device=gpu)) and fb.state_dict()["_growth_tracker"] == 1


# ------------------------------------------------------------------ 8. Masking.step(clip_grad=...)
def test_masking_step_with_clip_grad(gpu):
    from make_golden import TinyNet
    from slak_amd.optim_factory import MaskedAdamW
    from slak_amd.sparse_core import CosineDecay, Masking

    def make():
        torch.manual_seed(9)
        model = TinyNet(C=(6,), K=(13,))                    # two blocks at the smallest width the masking fixtures use
        for p in model.parameters():
            p.data = torch.randn_like(p) * 0.05
        model = model.to(gpu)
        opt = MaskedAdamW(model.parameters(), lr=1e-2, weight_decay=0.05)
        args = types.SimpleNamespace(device=str(gpu), fix=False, update_frequency=100, only_L=False, sparse_init="uniform", sparsity=0.4,
                                     distributed=False)
        torch.manual_seed(7)
        with contextlib.redirect_stdout(io.StringIO()):
            mask = Masking(opt, None, CosineDecay(0.3, 100), prune_rate=0.3, prune_mode="magnitude", growth_mode="gradient",
                           redistribution_mode="none", args=args)
            mask.add_module(model)
        return model, opt, mask
    (ma, oa, ka), (mb, ob, kb) = make(), make()
    gen = torch.Generator().manual_seed(6)
    grads = [(torch.randn(p.shape, generator=gen) * 0.1).to(gpu) for p in ma.parameters()]
    want = _norm64(grads, 1.0)
    for p, q, g in zip(ma.parameters(), mb.parameters(), grads):
        p.grad, q.grad = g.clone(), g.clone()
    norm = ka.step(clip_grad=1e9)                               # far above the norm: the update is step()'s
    assert kb.step() is None                                    # without the argument: as before
    assert ka.steps == kb.steps == 1
    assert norm.shape == () and _within_ulps(float(norm), want, 1)
    for p, q in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(p.detach(), q.detach())
    params = dict(ma.named_parameters())
    assert len(ka.masks) > 0
    for n, m in ka.masks.items():
        assert bool((params[n].detach()[m == 0] == 0).all()) and bool((params[n].detach()[m != 0] != 0).any())
    for p, g in zip(ma.parameters(), grads):
        p.grad = g.clone()
    norm = ka.step(clip_grad=0.5 * float(want))                 # clipping on: masks still applied
    assert ka.steps == 2 and oa.last_grad_control[1].item() < 1.0 and _within_ulps(float(norm), want, 1)
    for n, m in ka.masks.items():
        assert bool((params[n].detach()[m == 0] == 0).all())
    kb.optimizer = torch.optim.SGD(mb.parameters(), lr=0.1)
    with pytest.raises(RuntimeError):
        kb.step(clip_grad=1.0)                                  # no MaskedAdamW bound: refuse, do not fall back
