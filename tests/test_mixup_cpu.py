"""slak_amd.mixup without a GPU: timm's Mixup surface (timm1/data/mixup.py:90-218), every seeded reference run of tests/golden/mixup_*.npz
(tests/golden/make_mixup_golden.py) reproduced BIT FOR BIT on CPU tensors -- mixed batch, target and the position of the host random stream -- and the
host-side answers of the two entry points (`*_supported`, status codes before anything touches a GPU)."""
import ast
import ctypes
import glob
import inspect
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

FIXTURES = sorted(os.path.basename(p)[len("mixup_"):-4] for p in glob.glob(os.path.join(GOLDEN, "mixup_*.npz")))
EXPECTED = ["batch_cutmix_only", "batch_minmax", "batch_mixup_only", "batch_no_correct_lam", "batch_prob0", "batch_recipe", "elem_prob05", "elem_recipe",
            "pair_recipe"]


def test_all_nine_fixtures_are_present():
    assert FIXTURES == EXPECTED
    assert sum(os.path.getsize(os.path.join(GOLDEN, "mixup_%s.npz" % n)) for n in FIXTURES) < 300 * 1024


def test_constructor_and_attribute_surface():
    from slak_amd.mixup import Mixup
    sig = inspect.signature(Mixup.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("mixup_alpha", 1.), ("cutmix_alpha", 0.), ("cutmix_minmax", None), ("prob", 1.0), ("switch_prob", 0.5), ("mode", "batch"),
        ("correct_lam", True), ("label_smoothing", 0.1), ("num_classes", 1000)]
    m = Mixup()
    assert (m.mixup_alpha, m.cutmix_alpha, m.cutmix_minmax, m.mix_prob, m.switch_prob, m.label_smoothing, m.num_classes, m.mode, m.correct_lam,
            m.mixup_enabled) == (1., 0., None, 1.0, 0.5, 0.1, 1000, "batch", True, True)
    m = Mixup(mixup_alpha=0.8, cutmix_alpha=0.3, cutmix_minmax=(0.2, 0.8), prob=0.7, switch_prob=0.4, mode="elem", correct_lam=False,
              label_smoothing=0.2, num_classes=11)                # main.py:296-299's keywords
    assert m.cutmix_alpha == 1.0 and m.cutmix_minmax == (0.2, 0.8)  # a min/max box pins the alpha
    assert (m.mixup_alpha, m.mix_prob, m.switch_prob, m.mode, m.correct_lam, m.label_smoothing, m.num_classes) == (0.8, 0.7, 0.4, "elem", False, 0.2, 11)
    with pytest.raises(AssertionError):
        Mixup(cutmix_minmax=(0.2, 0.5, 0.8))
    with pytest.raises(AssertionError):
        Mixup(mixup_alpha=0., cutmix_alpha=0., num_classes=11)(torch.zeros(2, 1, 2, 2), torch.zeros(2, dtype=torch.int64))


@pytest.mark.parametrize("name", EXPECTED)
def test_cpu_tensors_reproduce_the_reference_bit_for_bit(name):
    from slak_amd import mixup
    g = load_golden("mixup_" + name)
    fn = mixup.Mixup(**ast.literal_eval(str(g["cfg"])))
    x0, labels = torch.from_numpy(g["x0"]), torch.from_numpy(g["labels"])
    before = mixup.fused_hits
    np.random.seed(int(g["seed"]))
    for c in range(4):
        x = x0.clone()
        got_x, got_t = fn(x, labels)
        assert got_x is x                                        # in place, returned by identity
        assert got_t.dtype == torch.float32 and got_t.shape == (6, 11)
        assert np.array_equal(x.numpy().view(np.int32), g["x_%d" % c].view(np.int32)), (name, c)
        assert np.array_equal(got_t.numpy().view(np.int32), g["t_%d" % c].view(np.int32)), (name, c)
    assert np.random.rand() == float(g["tail"])                  # the stream stands where the reference left it
    assert mixup.fused_hits == before                            # CPU tensors never count as served by the kernels


def test_mixing_switched_off_draws_nothing_and_changes_nothing():
    from slak_amd.mixup import Mixup
    for mode in ("batch", "pair", "elem"):
        fn = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, label_smoothing=0.0, num_classes=5)
        fn.mixup_enabled = False
        x0 = torch.randn(4, 2, 3, 3)
        x, y = x0.clone(), torch.tensor([0, 4, 2, 2])
        np.random.seed(3)
        want = np.random.rand()
        np.random.seed(3)
        _, t = fn(x, y)
        assert np.random.rand() == want and torch.equal(x, x0)
        assert torch.equal(t, torch.nn.functional.one_hot(y, 5).float())


def test_odd_batch_asserts():
    from slak_amd import mixup
    with pytest.raises(AssertionError, match="even"):
        mixup.Mixup(num_classes=11)(torch.zeros(3, 1, 2, 2), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(AssertionError, match="even"):
        mixup.mix_(torch.zeros(3, 1, 2, 2), mixup.UNTOUCHED)


def test_lower_level_functions_on_cpu():
    """mix_ / soft_targets with explicit records against the formula written out here."""
    from slak_amd import mixup
    R = mixup.Record
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(4, 2, 5, 6, generator=g)
    recs = [R(mixup.MIX, 0.3, 0.7, 0, 0, 0, 0), R(mixup.CUTMIX, 0.5, 0.5, 1, 4, 2, 5), mixup.UNTOUCHED, R(mixup.CUTMIX, 1.0, 0.0, 2, 2, 0, 6)]
    x = x0.clone()
    assert mixup.mix_(x, recs) is x
    a, b = np.float32(0.3), np.float32(0.7)
    want = x0.clone()
    want[0] = x0[0] * a + x0[3] * b
    want[1][:, 1:4, 2:5] = x0[2][:, 1:4, 2:5]
    assert torch.equal(x, want)
    y = torch.tensor([1, 1, 0, 2])
    t = mixup.soft_targets(y, recs, 3, smoothing=0.1)
    off = 0.1 / 3
    on = 1. - 0.1 + off
    hot = lambda lab: torch.full((4, 3), off).scatter_(1, lab.view(-1, 1), on)
    ca = torch.tensor([0.3, 0.5, 1.0, 1.0]).unsqueeze(1)
    cb = torch.tensor([0.7, 0.5, 0.0, 0.0]).unsqueeze(1)
    assert torch.equal(t, hot(y) * ca + hot(y.flip(0)) * cb)
    with pytest.raises(ValueError):
        mixup.mix_(x0.clone(), recs[:3])                         # N records or one
    with pytest.raises(ValueError):
        mixup.mix_(x0.clone(), R(mixup.CUTMIX, 0.5, 0.5, 0, 6, 0, 6))    # box outside the 5 x 6 image
    with pytest.raises(ValueError):
        mixup.mix_(x0.clone(), R(7, 0.5, 0.5, 0, 0, 0, 0))


@pytest.fixture(scope="module")
def L():
    from slak_amd import build, _lib
    build.build()
    return _lib.lib()


def test_queries_and_status_codes_are_decided_on_the_host(L):
    from slak_amd import _lib
    F32, F16, BF16 = _lib.SLAK_F32, _lib.SLAK_F16, _lib.SLAK_BF16
    for dt, N, C, H, W, want in ((F32, 128, 3, 224, 224, 1), (F32, 2, 1, 1, 1, 1), (F32, 6, 3, 7, 9, 1), (F32, 3, 3, 7, 9, 0), (F32, 0, 3, 7, 9, 0),
                                 (F32, 1, 3, 7, 9, 0), (BF16, 6, 3, 7, 9, 0), (F16, 6, 3, 7, 9, 0), (9, 6, 3, 7, 9, 0), (F32, 6, 0, 7, 9, 0),
                                 (F32, 6, 3, 0, 9, 0), (F32, 6, 3, 7, 0, 0), (F32, 2, 4096, 512, 512, 0), (F32, 131072, 3, 7, 9, 0)):
        assert L.slak_mixup_images_supported(dt, N, C, H, W) == want, (dt, N, C, H, W)
    for N, K, want in ((128, 1000, 1), (2, 1, 1), (6, 21841, 1), (3, 11, 0), (0, 11, 0), (6, 0, 0), (2, 2 ** 30, 0)):
        assert L.slak_mixup_targets_supported(N, K) == want, (N, K)
    buf = ctypes.create_string_buffer(64)                        # never dereferenced: the argument checks come first, and no call below launches
    p = ctypes.cast(buf, ctypes.c_void_p)
    rec = _lib.MixupRecord(_lib.MIXUP_MIX, 0.5, 0.5, 0, 0, 0, 0)
    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
    img = lambda x=p, dt=F32, sh=rec, tab=None, N=6, C=3, H=7, W=9: L.slak_mixup_images(x, dt, sh, tab, N, C, H, W, None)
    assert img(x=None) == INV                                    # null pointers
    assert img(sh=None, tab=None) == INV and img(sh=rec, tab=p) == INV          # exactly one source of records
    assert img(N=0) == INV and img(N=-2) == INV and img(C=0) == INV and img(H=0) == INV and img(W=0) == INV
    assert img(dt=9) == INV
    assert img(N=3) == UNS and img(N=1) == UNS                   # N odd
    assert img(dt=BF16) == UNS and img(dt=F16) == UNS            # fp32 batches only
    assert img(N=2, C=4096, H=512, W=512) == UNS
    assert img(sh=_lib.MixupRecord(5, 0.5, 0.5, 0, 0, 0, 0)) == INV
    assert img(sh=_lib.MixupRecord(_lib.MIXUP_CUTMIX, 0.5, 0.5, 0, 8, 0, 9)) == INV and img(sh=_lib.MixupRecord(_lib.MIXUP_CUTMIX, 0.5, 0.5, 3, 2, 0, 9)) == INV
    assert img(sh=_lib.MixupRecord(_lib.MIXUP_NONE, 1.0, 0.0, 0, 0, 0, 0)) == _lib.OK      # nothing to do: answered without a launch
    assert img(sh=_lib.MixupRecord(_lib.MIXUP_CUTMIX, 1.0, 0.0, 3, 3, 0, 9)) == _lib.OK   # an empty box likewise
    tgt = lambda lab=p, sh=rec, tab=None, out=p, N=6, K=11: L.slak_mixup_targets(lab, sh, tab, 0.9, 0.01, out, N, K, None)
    assert tgt(lab=None) == INV and tgt(out=None) == INV
    assert tgt(sh=None) == INV and tgt(tab=p) == INV
    assert tgt(N=0) == INV and tgt(K=0) == INV and tgt(K=-1) == INV
    assert tgt(N=3) == UNS and tgt(N=2, K=2 ** 30) == UNS


def test_package_exports_mixup():
    import slak_amd
    from slak_amd import mixup
    assert "Mixup" in slak_amd.__all__ and slak_amd.Mixup is mixup.Mixup
    for n in ("Mixup", "Record", "mix_", "soft_targets", "rand_bbox", "rand_bbox_minmax", "cutmix_bbox_and_lam", "one_hot", "mixup_target"):
        assert n in mixup.__all__ and hasattr(mixup, n)
    assert not hasattr(mixup, "FastCollateMixup")                # collate-time CPU work: out of scope
