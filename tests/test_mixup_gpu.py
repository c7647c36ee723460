"""slak_amd.mixup on the device: the two HIP launches (slak_mixup_images / slak_mixup_targets) against the seeded reference runs of
tests/golden/mixup_*.npz and against the reference's op sequence as torch ops -- every comparison is EXACT (the op sequence and the roundings are the
reference's: two rounded multiplies and an add, CutMix copies bits), so there is no tolerance anywhere in this file."""
import ast
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURES = ["batch_recipe", "batch_mixup_only", "batch_cutmix_only", "batch_minmax", "batch_no_correct_lam", "batch_prob0", "pair_recipe", "elem_recipe",
            "elem_prob05"]
SHAPES = [(2, 3, 7, 9), (6, 3, 7, 9), (8, 3, 32, 32), (4, 3, 64, 80), (2, 1, 1, 1)]
CLASSES = [11, 1000, 1001]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _formula(x0, recs):
    """timm1/data/mixup.py:159-194 from explicit records: every image from the ORIGINALS (a copy of the batch), plain torch ops."""
    from slak_amd import mixup
    if isinstance(recs, mixup.Record):
        recs = [recs] * len(x0)
    out = x0.clone()
    for n, r in enumerate(recs):
        j = len(x0) - 1 - n
        if r.kind == mixup.MIX:
            out[n] = x0[n] * float(np.float32(r.a)) + x0[j] * float(np.float32(r.b))
        elif r.kind == mixup.CUTMIX:
            out[n][:, r.yl:r.yh, r.xl:r.xh] = x0[j][:, r.yl:r.yh, r.xl:r.xh]
    return out


def _targets_formula(y, recs, K, smoothing):
    """timm1/data/mixup.py:17-27 with the columns found by comparison (so that a label outside [0, K) has an answer): v(y_n) a_n + v(y_j) b_n."""
    from slak_amd import mixup
    if isinstance(recs, mixup.Record):
        recs = [recs] * len(y)
    off = smoothing / K
    on = 1. - smoothing + off
    hot = torch.where(torch.arange(K, device=y.device)[None, :] == y[:, None], torch.tensor(on, dtype=torch.float32, device=y.device),
                      torch.tensor(off, dtype=torch.float32, device=y.device))
    a = torch.tensor([float(np.float32(r.a)) for r in recs], dtype=torch.float32, device=y.device)[:, None]
    b = torch.tensor([float(np.float32(r.b)) for r in recs], dtype=torch.float32, device=y.device)[:, None]
    return hot * a + hot.flip(0) * b


def _batch(shape, gpu, seed=0):
    g = torch.Generator(device=gpu).manual_seed(seed)
    return torch.randn(*shape, device=gpu, generator=g)


@pytest.fixture
def no_kernels(monkeypatch):
    """Routes every call to the torch formula, whatever the tensors are."""
    from slak_amd import mixup

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            m.setattr(mixup, "_images_ok", lambda x: False)
            m.setattr(mixup, "_labels_ok", lambda *a: False)
            yield
    return off


# ================================================================ the seeded reference runs
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_bit_for_bit_on_the_device(name, gpu):
    from slak_amd import mixup
    g = load_golden("mixup_" + name)
    fn = mixup.Mixup(**ast.literal_eval(str(g["cfg"])))
    x0, labels = torch.from_numpy(g["x0"]).to(gpu), torch.from_numpy(g["labels"]).to(gpu)
    np.random.seed(int(g["seed"]))
    for c in range(4):
        hits = mixup.fused_hits
        x = x0.clone()
        got_x, got_t = fn(x, labels)
        assert got_x is x and mixup.fused_hits == hits + 1
        assert got_t.dtype == torch.float32 and got_t.is_cuda and got_t.shape == (6, 11)
        assert np.array_equal(x.cpu().numpy().view(np.int32), g["x_%d" % c].view(np.int32)), (name, c)
        assert np.array_equal(got_t.cpu().numpy().view(np.int32), g["t_%d" % c].view(np.int32)), (name, c)
    assert np.random.rand() == float(g["tail"])


# ================================================================ kernel against the torch formula, from the same seed
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_kernel_equals_the_formula(mode, shape, gpu, no_kernels):
    from slak_amd import mixup
    x0 = _batch(shape, gpu, seed=sum(shape))
    for call, K in enumerate(CLASSES * 2):                       # six calls: both kinds come up in every mode
        fn = mixup.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=K, mode=mode)
        y = torch.randint(0, K, (shape[0],), generator=torch.Generator().manual_seed(call)).to(gpu)
        hits = mixup.fused_hits
        np.random.seed(40 + call)
        x = x0.clone()
        _, t = fn(x, y)
        tail = np.random.rand()
        assert mixup.fused_hits == hits + 1
        with no_kernels():
            np.random.seed(40 + call)
            xr = x0.clone()
            _, tr = fn(xr, y)
            assert np.random.rand() == tail
        assert mixup.fused_hits == hits + 1
        assert _same_bits(x, xr), (mode, shape, call)
        assert _same_bits(t, tr), (mode, shape, K)


# ================================================================ forced boxes and coefficients
def _boxes(H, W):
    return {"empty_rows": (3, 3, 1, W), "empty_cols": (0, H, 4, 4), "whole": (0, H, 0, W), "one_pixel": (H // 2, H // 2 + 1, 3, 4),
            "top": (0, 2, 2, W - 1), "bottom": (H - 3, H, 1, W - 2), "left": (1, H - 1, 0, 3), "right": (2, H - 1, W - 4, W),
            "odd_xl": (1, H - 2, 3, W - 1), "corner": (H - 1, H, W - 1, W)}


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (6, 3, 7, 9), (4, 3, 64, 80)], ids=lambda s: "x".join(map(str, s)))
def test_forced_boxes(shape, gpu):
    from slak_amd import mixup
    N, C, H, W = shape
    x0 = _batch(shape, gpu, seed=3)
    for name, box in _boxes(H, W).items():
        shared = mixup.Record(mixup.CUTMIX, 0.4, 0.6, *box)
        hits = mixup.fused_hits
        x = x0.clone()
        assert mixup.mix_(x, shared) is x and mixup.fused_hits == hits + 1
        want = _formula(x0, shared)
        assert _same_bits(x, want), ("shared", name)
        if name.startswith("empty"):
            assert _same_bits(x, x0)
        if name == "whole":
            assert _same_bits(x, x0.flip(0))
        # the same box on ONE image of a table, its partner untouched, the other pairs mixed
        recs = [mixup.Record(mixup.MIX, 0.25 + 0.1 * n, 0.75 - 0.1 * n, 0, 0, 0, 0) for n in range(N)]
        recs[0], recs[N - 1] = shared, mixup.UNTOUCHED
        x = x0.clone()
        mixup.mix_(x, recs)
        assert _same_bits(x, _formula(x0, recs)), ("table", name)
        assert _same_bits(x[N - 1], x0[N - 1])


def test_overlapping_boxes_and_different_coefficients_in_one_pair(gpu):
    """The in-place hazard: both images of the pair are rewritten from both originals."""
    from slak_amd import mixup
    R = mixup.Record
    for shape in ((2, 3, 7, 9), (2, 3, 64, 80)):
        H, W = shape[2:]
        x0 = _batch(shape, gpu, seed=8)
        for recs in ([R(mixup.CUTMIX, 0.5, 0.5, 1, H - 2, 1, W - 3), R(mixup.CUTMIX, 0.6, 0.4, 3, H, 4, W)],
                     [R(mixup.MIX, 0.3, 0.7, 0, 0, 0, 0), R(mixup.MIX, 0.9, 0.1, 0, 0, 0, 0)],
                     [R(mixup.MIX, 0.3, 0.7, 0, 0, 0, 0), R(mixup.CUTMIX, 0.6, 0.4, 2, H - 1, 3, W - 2)],
                     [R(mixup.CUTMIX, 0.6, 0.4, 0, 4, 0, 5), R(mixup.MIX, 0.2, 0.8, 0, 0, 0, 0)]):
            x = x0.clone()
            mixup.mix_(x, recs)
            assert _same_bits(x, _formula(x0, recs)), (shape, recs)
            assert not _same_bits(x[0], x0[0]) and not _same_bits(x[1], x0[1])


def test_non_finite_values_stay_where_they_are(gpu):
    from slak_amd import mixup
    R = mixup.Record
    N, C, H, W = 4, 3, 7, 9
    box = (2, 5, 3, 7)
    x0 = _batch((N, C, H, W), gpu, seed=5)
    inside = torch.zeros(H, W, dtype=torch.bool, device=gpu)
    inside[box[0]:box[1], box[2]:box[3]] = True
    fill = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0], device=gpu).repeat(C * H * W // 4 + 1)[:C * H * W].view(C, H, W)
    x0[3] = torch.where(inside, x0[3], fill)                     # the partner of image 0: non-finite and -0.0 everywhere outside the box
    x0[0, 0, 0, 0] = -0.0
    # a cutmix image next to an untouched partner; the other pair is mixed
    recs = [R(mixup.CUTMIX, 0.5, 0.5, *box), R(mixup.MIX, 0.3, 0.7, 0, 0, 0, 0), R(mixup.MIX, 0.6, 0.4, 0, 0, 0, 0), mixup.UNTOUCHED]
    x = x0.clone()
    mixup.mix_(x, recs)
    assert _same_bits(x[3], x0[3])                               # untouched: every bit, the -0.0s included
    assert torch.equal(_bits(x[0])[:, ~inside], _bits(x0[0])[:, ~inside])       # outside the box: image 0's own bits
    assert torch.equal(_bits(x[0])[:, inside], _bits(x0[3])[:, inside])         # inside: the partner's bits
    assert torch.isfinite(x[0]).all() and torch.isfinite(x[1]).all() and torch.isfinite(x[2]).all()    # nothing crossed into the other pair
    assert _same_bits(x[1:3], _formula(x0, recs)[1:3])
    # the whole batch under one cutmix record (batch mode): images 0 and 3 swap their boxes, nothing else moves
    x = x0.clone()
    mixup.mix_(x, R(mixup.CUTMIX, 0.5, 0.5, *box))
    assert torch.equal(_bits(x)[:, :, ~inside], _bits(x0)[:, :, ~inside])
    assert torch.equal(_bits(x)[:, :, inside], _bits(x0.flip(0))[:, :, inside])
    # a cutmix image whose partner is MIXED (the whole-image pass): still its own bits outside the box
    recs = [R(mixup.CUTMIX, 0.5, 0.5, *box), mixup.UNTOUCHED, mixup.UNTOUCHED, R(mixup.MIX, 0.5, 0.5, 0, 0, 0, 0)]
    x = x0.clone()
    mixup.mix_(x, recs)
    assert torch.equal(_bits(x[0])[:, ~inside], _bits(x0[0])[:, ~inside]) and torch.equal(_bits(x[0])[:, inside], _bits(x0[3])[:, inside])
    assert _same_bits(x[1:3], x0[1:3])
    want = _formula(x0, recs)[3]
    assert torch.equal(torch.isnan(x[3]), torch.isnan(want))
    assert torch.equal(_bits(torch.nan_to_num(x[3], nan=1.0)), _bits(torch.nan_to_num(want, nan=1.0)))
    # lam == 1 through the class: nothing moves
    fn = mixup.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0, num_classes=5)
    x = x0.clone()
    fn(x, torch.zeros(N, dtype=torch.int64, device=gpu))
    assert _same_bits(x, x0)


def test_labels(gpu):
    from slak_amd import mixup
    R = mixup.Record
    for K in CLASSES:
        y = torch.tensor([3, 5, K - 1, 0, 5, 3], device=gpu)     # pairs (0, 5) and (1, 4) carry equal labels
        recs = [R(mixup.MIX, 0.3, 0.7, 0, 0, 0, 0), R(mixup.CUTMIX, 0.5625, 0.4375, 0, 1, 0, 1), mixup.UNTOUCHED, R(mixup.MIX, 0.9, 0.1, 0, 0, 0, 0),
                R(mixup.MIX, 0.2, 0.8, 0, 0, 0, 0), R(mixup.MIX, 0.45, 0.55, 0, 0, 0, 0)]
        for smoothing in (0.1, 0.0):
            hits = mixup.fused_hits
            t = mixup.soft_targets(y, recs, K, smoothing)
            assert mixup.fused_hits == hits + 1 and t.shape == (6, K) and t.dtype == torch.float32
            assert _same_bits(t, _targets_formula(y, recs, K, smoothing)), (K, smoothing)
            off = np.float32(smoothing / K)
            on = np.float32(1. - smoothing + smoothing / K)
            assert t[0, 3].item() == np.float32(on * np.float32(0.3)) + np.float32(on * np.float32(0.7))       # both terms on one column
            assert t[0, 4].item() == np.float32(off * np.float32(0.3)) + np.float32(off * np.float32(0.7))
            shared = R(mixup.MIX, 0.35, 0.65, 0, 0, 0, 0)
            assert _same_bits(mixup.soft_targets(y, shared, K, smoothing), _targets_formula(y, shared, K, smoothing))
        # labels outside [0, K): they match no column -- off-values for their term, and no fault
        bad = torch.tensor([K, -1, 2, 2 ** 40, -2 ** 62, 7], device=gpu)
        t = mixup.soft_targets(bad, recs, K, 0.1)
        torch.cuda.synchronize()
        assert _same_bits(t, _targets_formula(bad, recs, K, 0.1))
        off = float(np.float32(0.1 / K))
        assert torch.all(t[1] == np.float32(np.float32(off * np.float32(0.5625)) + np.float32(off * np.float32(0.4375))))   # both labels of that row are outside


def test_two_runs_give_identical_bits(gpu):
    from slak_amd import mixup
    x0 = _batch((8, 3, 32, 32), gpu, seed=2)
    y = torch.arange(8, device=gpu)
    for mode in ("batch", "pair", "elem"):
        fn = mixup.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=1001, mode=mode)
        runs = []
        for _ in range(2):
            np.random.seed(12)
            x = x0.clone()
            runs.append((x, fn(x, y)[1]))
        assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])


def test_what_the_kernels_do_not_take_runs_the_formula(gpu):
    from slak_amd import mixup
    y = torch.tensor([1, 0, 3, 2, 2, 5], device=gpu)
    base = _batch((6, 3, 7, 12), gpu, seed=6)
    for mode in ("batch", "elem"):
        fn = mixup.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=11, mode=mode)
        # the reference's result on the same fp32 values, from a contiguous batch on the kernels
        np.random.seed(21)
        want_x = base[:, :, :, :9].contiguous()
        _, want_t = fn(want_x, y)
        hits = mixup.fused_hits
        np.random.seed(21)
        view = base.clone()[:, :, :, :9]                         # not contiguous
        got_x, got_t = fn(view, y)
        assert got_x is view and mixup.fused_hits == hits
        assert _same_bits(view, want_x) and _same_bits(got_t, want_t)
        # bf16 images: the formula in bf16, as the reference would run it (two calls from one seed agree; fp32 targets)
        np.random.seed(22)
        h0 = base.to(torch.bfloat16)
        h = h0.clone()
        _, th = fn(h, y)
        assert mixup.fused_hits == hits and h.dtype == torch.bfloat16 and th.dtype == torch.float32
        np.random.seed(22)
        shared, table = fn._draw(h0.shape)
        assert torch.equal(h.view(torch.int16), _formula(h0, shared if table is None else table).view(torch.int16))
        # int32 labels: the formula as well
        np.random.seed(23)
        x = want_x.clone()
        _, t32 = fn(x, y.to(torch.int32))
        assert mixup.fused_hits == hits
        np.random.seed(23)
        x2 = want_x.clone()
        _, t64 = fn(x2, y)
        assert mixup.fused_hits == hits + 1 and _same_bits(x, x2) and _same_bits(t32, t64)


# ================================================================ end to end
def test_small_model_trains_the_same_on_kernels_and_formula(gpu, no_kernels):
    """Mixup + SoftTargetCrossEntropy under bf16 autocast with MaskedAdamW, three steps: finite and identical losses from the same seeds."""
    import slak_amd
    import slak_amd.slak_model as M
    from slak_amd import block_ops, mixup
    from slak_amd.optim_factory import MaskedAdamW
    saved = (M.Block.fused_tail, M.ReparamLargeKernelConv.fused_bn, M.ReparamLargeKernelConv.fused_tri, M.Block.fused_block, M.LayerNorm.fused_cf,
             block_ops.cache_lowp_weights, M.use_sync_bn)
    M.use_sync_bn = False
    M.Block.fused_tail = M.ReparamLargeKernelConv.fused_bn = M.ReparamLargeKernelConv.fused_tri = M.Block.fused_block = M.LayerNorm.fused_cf = True
    block_ops.cache_lowp_weights = True
    try:
        torch.manual_seed(3)
        net0 = M.SLaK(in_chans=3, num_classes=10, depths=[1, 1, 2, 1], dims=[10, 21, 43, 86], drop_path_rate=0.0, kernel_size=[13, 13, 9, 7, 5],
                      Decom=True, bn=True, lowp_dwconv=True).to(gpu)
        xs = _batch((4, 3, 64, 64), gpu, seed=11)
        ys = torch.tensor([1, 7, 7, 4], device=gpu)
        crit = slak_amd.SoftTargetCrossEntropy()

        def run():
            net = copy.deepcopy(net0)
            opt = MaskedAdamW(net.parameters(), lr=1e-3)
            fn = mixup.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=10)
            np.random.seed(5)
            losses = []
            for _ in range(3):
                samples, targets = fn(xs.clone(), ys)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    loss = crit(net(samples), targets)
                loss.backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
                losses.append(float(loss.item()))
            return losses
        hits = mixup.fused_hits
        on_kernels = run()
        assert mixup.fused_hits == hits + 3
        with no_kernels():
            on_formula = run()
        assert mixup.fused_hits == hits + 3
    finally:
        (M.Block.fused_tail, M.ReparamLargeKernelConv.fused_bn, M.ReparamLargeKernelConv.fused_tri, M.Block.fused_block, M.LayerNorm.fused_cf,
         block_ops.cache_lowp_weights, M.use_sync_bn) = saved
    assert np.isfinite(on_kernels).all() and np.isfinite(on_formula).all()
    assert on_kernels == on_formula, (on_kernels, on_formula)


def test_fused_criterion_loss_can_be_divided_in_place(gpu):
    """engine.py:79 runs ``loss /= update_freq`` on what the criterion returned: the fused criterion must hand out a tensor of its own, not a view."""
    import slak_amd
    from slak_amd import loss as LS, mixup
    x = _batch((4, 11), gpu, seed=1).requires_grad_(True)
    t = mixup.soft_targets(torch.tensor([1, 0, 3, 3], device=gpu), mixup.Record(mixup.MIX, 0.3, 0.7, 0, 0, 0, 0), 11, 0.1)
    hits = LS.fused_hits
    loss = slak_amd.SoftTargetCrossEntropy()(x, t)
    assert LS.fused_hits == hits + 1
    whole = float(loss.detach())
    loss /= 2
    loss.backward()
    xr = x.detach().clone().requires_grad_(True)
    ref = torch.sum(-t * torch.log_softmax(xr, -1), -1).mean()
    (ref / 2).backward()
    assert abs(float(loss.detach()) - whole / 2) <= 1e-7 * abs(whole) and abs(whole - float(ref.detach())) <= 1e-5 * abs(whole)
    assert torch.allclose(x.grad, xr.grad, rtol=1e-4, atol=1e-6)


def test_reference_train_one_epoch_with_mixup_fn(gpu):
    """engine.py:46-58: the reference's unmodified train_one_epoch (oracle.ref_modules.load_engine, set up as tests/test_reference_engine_gpu.py sets it
    up) with ``mixup_fn=slak_amd.mixup.Mixup(...)`` and SoftTargetCrossEntropy: every batch is mixed on the kernels, every loss is finite."""
    import slak_amd
    import test_reference_engine_gpu as E
    from slak_amd import mixup
    engine, utils = E._engine()
    g = load_golden("engine_uf1")
    model = E._model(g, gpu)
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        args, model_ema, optimizer, lr_values, wd_values, _, loader, mask, steps_per_epoch = E._construct(g, gpu, utils, 1, model)
    num_classes = ast.literal_eval(str(g["cfg"]))["num_classes"]
    fn = mixup.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1,
                     num_classes=num_classes)                    # main.py:296-299
    seen = []

    class Criterion(slak_amd.SoftTargetCrossEntropy):            # main.py:397-399, keeping what it saw
        def forward(self, x, target):
            loss = super().forward(x, target)
            seen.append((tuple(target.shape), target.dtype, float(target.sum(-1).min()), float(loss.detach())))
            return loss
    hits = mixup.fused_hits
    np.random.seed(2)
    with contextlib.redirect_stdout(sink):
        train_stats = engine.train_one_epoch(
            model, Criterion(), loader, optimizer,
            gpu, 0, None, args.clip_grad, model_ema, fn,
            log_writer=None, wandb_logger=None, start_steps=0,
            lr_schedule_values=lr_values, wd_schedule_values=wd_values,
            num_training_steps_per_epoch=steps_per_epoch, update_freq=1,
            use_amp=False, mask=mask
        )
    assert len(seen) == len(loader) and mixup.fused_hits == hits + len(loader)
    batch = loader[0][0].shape[0]
    for shape, dtype, rowsum, loss in seen:
        assert shape == (batch, num_classes) and dtype == torch.float32 and abs(rowsum - 1.0) < 1e-5 and np.isfinite(loss)
    assert np.isfinite(train_stats["loss"]) and mask.steps == steps_per_epoch
