"""Mixup / CutMix of a batch on two HIP launches (slak_mixup_images / slak_mixup_targets, csrc/mixup.hip), behind timm's ``Mixup`` surface.

The reference builds ``Mixup(mixup_alpha=..., cutmix_alpha=..., cutmix_minmax=..., prob=..., switch_prob=..., mode=..., label_smoothing=...,
num_classes=...)`` from ``timm.data.mixup`` (main.py:21, 296-299; every README recipe: ``--mixup 0.8 --cutmix 1.0 --smoothing 0.1``) and calls it
on every batch on the device before the forward (engine.py:49-50); the criterion is then ``SoftTargetCrossEntropy`` (main.py:397-399,
slak_amd.loss).  ``Mixup`` here has the same constructor, attributes and ``__call__(x, target) -> (x, target)`` (timm1/data/mixup.py:90-218):
``x`` is mixed in place and returned by identity, ``target`` becomes the (N, K) float32 distribution.

Random numbers.  Every parameter is drawn from the HOST generator with the same ``np.random`` calls in the same order as the reference
(``_params_per_batch``, ``_params_per_elem``, ``rand_bbox``, ``rand_bbox_minmax``, ``cutmix_bbox_and_lam``), BEFORE anything touches the batch
(no draw depends on it): a seed gives the reference's parameters and leaves the stream where the reference leaves it -- the rule ``Masking``'s
random growth follows.  The draws end in per-image ``Record``s (kind, the fp32 coefficients a / b, the box); the coefficients are evaluated as
the reference evaluates them -- 'batch': ``float32(lam)`` and ``float32(1. - lam)`` with the subtraction in double (lam is a Python float there);
'pair' / 'elem': lam is ``np.float32`` and b = ``float32(1) - lam``; after a CutMix box correction lam is the corrected value rounded to fp32.

Device work.  ``mix_`` and ``soft_targets`` take records and run one launch each on contiguous NCHW float32 CUDA batches with int64 labels;
'batch' mode passes its one record by value (no copy to the device), 'pair' / 'elem' stage N records in pinned memory with one non-blocking
copy.  Nothing synchronises with the host.  Anything else -- CPU tensors, another dtype, a non-contiguous batch, labels that are not an int64
(N,) tensor on the batch's device -- runs the reference's op sequence as torch ops from the SAME records: the result never depends silently on
which path ran, and ``fused_hits`` counts the calls the kernels served.  ``FastCollateMixup`` (collate-time CPU work) is not provided.
"""
import collections

import numpy as np
import torch

from . import _lib

__all__ = ["Mixup", "Record", "mix_", "soft_targets", "one_hot", "mixup_target", "rand_bbox", "rand_bbox_minmax", "cutmix_bbox_and_lam",
           "NONE", "MIX", "CUTMIX", "UNTOUCHED"]

fused_hits = 0                # calls (Mixup.__call__, mix_, soft_targets) the HIP kernels served so far (tests, tools/time_mixup.py)
NONE, MIX, CUTMIX = _lib.MIXUP_NONE, _lib.MIXUP_MIX, _lib.MIXUP_CUTMIX

Record = collections.namedtuple("Record", "kind a b yl yh xl xh")
Record.__doc__ = """What happens to one image (slak_mixup_record_t): ``kind`` NONE / MIX (x a + partner b) / CUTMIX (partner's box copied in), the fp32
coefficients ``a`` (own) and ``b`` (partner) -- the target row's coefficients for every kind -- and the box rows [yl, yh), columns [xl, xh)."""
UNTOUCHED = Record(NONE, np.float32(1.0), np.float32(0.0), 0, 0, 0, 0)

_REC_DTYPE = np.dtype([("kind", "<i4"), ("a", "<f4"), ("b", "<f4"), ("yl", "<i4"), ("yh", "<i4"), ("xl", "<i4"), ("xh", "<i4")])
assert _REC_DTYPE.itemsize == 28


# ------------------------------------------------------------------------------------------------ host draws (timm1/data/mixup.py:30-87)
def rand_bbox(img_shape, lam, margin=0., count=None):
    """timm1/data/mixup.py:30-51: a box of area ratio 1 - lam around a uniform centre, clipped to the image.  Draws: centre row, centre column."""
    H, W = img_shape[-2:]
    side = np.sqrt(1 - lam)
    bh, bw = int(H * side), int(W * side)
    my, mx = int(margin * bh), int(margin * bw)
    cy = np.random.randint(0 + my, H - my, size=count)
    cx = np.random.randint(0 + mx, W - mx, size=count)
    return np.clip(cy - bh // 2, 0, H), np.clip(cy + bh // 2, 0, H), np.clip(cx - bw // 2, 0, W), np.clip(cx + bw // 2, 0, W)


def rand_bbox_minmax(img_shape, minmax, count=None):
    """timm1/data/mixup.py:54-74: box height and width uniform between the two image ratios.  Draws: height, width, top row, left column."""
    assert len(minmax) == 2
    H, W = img_shape[-2:]
    bh = np.random.randint(int(H * minmax[0]), int(H * minmax[1]), size=count)
    bw = np.random.randint(int(W * minmax[0]), int(W * minmax[1]), size=count)
    top = np.random.randint(0, H - bh, size=count)
    left = np.random.randint(0, W - bw, size=count)
    return top, top + bh, left, left + bw


def cutmix_bbox_and_lam(img_shape, lam, ratio_minmax=None, correct_lam=True, count=None):
    """timm1/data/mixup.py:77-87: the box and, with ``correct_lam`` or a min/max box, lam recomputed from the box that survived the clipping."""
    box = rand_bbox_minmax(img_shape, ratio_minmax, count=count) if ratio_minmax is not None else rand_bbox(img_shape, lam, count=count)
    if correct_lam or ratio_minmax is not None:
        yl, yh, xl, xh = box
        lam = 1. - (yh - yl) * (xh - xl) / float(img_shape[-2] * img_shape[-1])
    return box, lam


# ------------------------------------------------------------------------------------------------ the torch formulas (timm1/data/mixup.py:17-27, 159-207)
def one_hot(x, num_classes, on_value=1., off_value=0., device='cuda'):
    """timm1/data/mixup.py:17-19."""
    idx = x.long().view(-1, 1)
    return torch.full((idx.size()[0], num_classes), off_value, device=device).scatter_(1, idx, on_value)


def _on_off(num_classes, smoothing):
    off = smoothing / num_classes                               # in double; torch.full / scatter_ (and the kernel's caller) round once
    return 1. - smoothing + off, off


def mixup_target(target, num_classes, lam=1., smoothing=0.0, device='cuda'):
    """timm1/data/mixup.py:22-27."""
    on, off = _on_off(num_classes, smoothing)
    own = one_hot(target, num_classes, on_value=on, off_value=off, device=device)
    partner = one_hot(target.flip(0), num_classes, on_value=on, off_value=off, device=device)
    return own * lam + partner * (1. - lam)


def _targets_formula(labels, a, b, num_classes, smoothing, device):
    """mixup_target with the two coefficients given: Python floats ('batch') or (N, 1) tensors."""
    on, off = _on_off(num_classes, smoothing)
    own = one_hot(labels, num_classes, on_value=on, off_value=off, device=device)
    partner = one_hot(labels.flip(0), num_classes, on_value=on, off_value=off, device=device)
    return own * a + partner * b


def _mix_formula(x, shared, table):
    """The image pass as torch ops.  One shared record: _mix_batch's sequence (timm1/data/mixup.py:196-207); a table: _mix_elem / _mix_pair's loop
    over a clone of the batch (:159-194)."""
    if shared is not None:
        if shared.kind == MIX:
            other = x.flip(0).mul_(float(shared.b))
            x.mul_(float(shared.a)).add_(other)
        elif shared.kind == CUTMIX:
            yl, yh, xl, xh = shared[3:]
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        return x
    src = x.clone()
    for n, r in enumerate(table):
        j = len(table) - 1 - n
        if r.kind == MIX:
            x[n] = src[n] * r.a + src[j] * r.b                  # np.float32 scalars, as in the reference
        elif r.kind == CUTMIX:
            x[n][:, r.yl:r.yh, r.xl:r.xh] = src[j][:, r.yl:r.yh, r.xl:r.xh]
    return x


# ------------------------------------------------------------------------------------------------ records -> launches
def _records(records, N, H, W):
    """(shared, table): one checked Record, or a list of N."""
    def checked(r):
        r = Record(*r)
        if r.kind not in (NONE, MIX, CUTMIX) or not (0 <= r.yl <= r.yh <= H and 0 <= r.xl <= r.xh <= W):
            raise ValueError("bad mixup record for a %d x %d image: %r" % (H, W, (r,)))
        return Record(int(r.kind), np.float32(r.a), np.float32(r.b), int(r.yl), int(r.yh), int(r.xl), int(r.xh))
    if isinstance(records, Record) or (len(records) == 7 and not isinstance(records[0], (tuple, list))):
        return checked(records), None
    if len(records) != N:
        raise ValueError("%d mixup records for a batch of %d" % (len(records), N))
    return None, [checked(r) for r in records]


class _Staged:
    """The records in the form the entry points take: a host struct for a shared record, else a device table (pinned staging, one non-blocking copy)."""

    def __init__(self, shared, table, device):
        self.shared = self.table = None
        if shared is not None:
            self.shared = _lib.MixupRecord(shared.kind, float(shared.a), float(shared.b), shared.yl, shared.yh, shared.xl, shared.xh)
        else:
            host = torch.from_numpy(np.array([tuple(r) for r in table], dtype=_REC_DTYPE).view(np.uint8)).pin_memory()
            self.table = host.to(device, non_blocking=True)

    def args(self):
        return (self.shared, None) if self.shared is not None else (None, self.table.data_ptr())


def _images_ok(x):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and not x.requires_grad):
        return False
    return bool(_lib.lib().slak_mixup_images_supported(_lib.SLAK_F32, *x.shape))


def _labels_ok(labels, N, device, K):
    if not (isinstance(labels, torch.Tensor) and labels.dtype == torch.int64 and labels.shape == (N,) and labels.device == device and labels.is_cuda):
        return False
    return bool(_lib.lib().slak_mixup_targets_supported(N, K))


def _mix_launch(x, staged):
    from .ops import _stream, _on
    N, C, H, W = x.shape
    with _on(x.device):
        _lib.check(_lib.lib().slak_mixup_images(x.data_ptr(), _lib.SLAK_F32, *staged.args(), N, C, H, W, _stream(x.device)), "slak_mixup_images")
    return x


def _targets_launch(labels, staged, num_classes, smoothing):
    from .ops import _stream, _on
    labels = labels.contiguous()
    N = labels.shape[0]
    on, off = _on_off(num_classes, smoothing)
    out = torch.empty((N, num_classes), dtype=torch.float32, device=labels.device)
    with _on(labels.device):
        _lib.check(_lib.lib().slak_mixup_targets(labels.data_ptr(), *staged.args(), on, off, out.data_ptr(), N, num_classes, _stream(labels.device)),
                   "slak_mixup_targets")
    return out


def mix_(x, records):
    """Mix the batch ``x`` (N, C, H, W) IN PLACE under ``records`` -- one ``Record`` every image shares, or a sequence of N -- and return it.
    Image n is mixed with the ORIGINAL of image N-1-n.  One launch on a contiguous float32 CUDA batch; the same result as torch ops elsewhere."""
    global fused_hits
    assert len(x) % 2 == 0, 'Batch size should be even when using this'
    shared, table = _records(records, len(x), x.shape[-2], x.shape[-1])
    if _images_ok(x):
        _mix_launch(x, _Staged(shared, table, x.device))
        fused_hits += 1
        return x
    return _mix_formula(x, shared, table)


def soft_targets(labels, records, num_classes, smoothing=0.0):
    """``labels`` (N,) -> float32 (N, num_classes): row n = one_hot(y_n) a_n + one_hot(y_{N-1-n}) b_n with the on / off values of label smoothing
    (timm1/data/mixup.py:22-27).  One launch for int64 CUDA labels.  A label outside [0, num_classes) gives a row of off-values on the launch;
    the torch formula (``scatter_``) refuses it."""
    global fused_hits
    N = len(labels)
    assert N % 2 == 0, 'Batch size should be even when using this'
    shared, table = _records(records, N, 2 ** 31 - 1, 2 ** 31 - 1)
    if isinstance(labels, torch.Tensor) and _labels_ok(labels, N, labels.device, num_classes):
        out = _targets_launch(labels, _Staged(shared, table, labels.device), num_classes, smoothing)
        fused_hits += 1
        return out
    if shared is not None:
        return _targets_formula(labels, float(shared.a), float(shared.b), num_classes, smoothing, labels.device)
    col = lambda v: torch.tensor(np.array(v, dtype=np.float32), device=labels.device).unsqueeze(1)
    return _targets_formula(labels, col([r.a for r in table]), col([r.b for r in table]), num_classes, smoothing, labels.device)


# ------------------------------------------------------------------------------------------------ timm1/data/mixup.py:90-218
class Mixup:
    """Mixup / CutMix with one set of parameters per batch, per pair of images or per image (timm1/data/mixup.py:90-218).

    Args:
        mixup_alpha (float): Beta parameter of mixup's lam; mixup is active if > 0.
        cutmix_alpha (float): Beta parameter of CutMix's lam; CutMix is active if > 0.
        cutmix_minmax (List[float]): box sides as min / max ratios of the image sides; CutMix is active and ignores its alpha if not None.
        prob (float): probability of mixing a batch ('batch') or an element ('pair' / 'elem').
        switch_prob (float): probability of CutMix where both are active.
        mode (str): 'batch', 'pair' (a pair of images shares its parameters) or 'elem'.
        correct_lam (bool): recompute lam from the box that is left after clipping at the image borders.
        label_smoothing (float): label smoothing of the mixed target.
        num_classes (int): number of classes of the target.
    """

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5,
                 mode='batch', correct_lam=True, label_smoothing=0.1, num_classes=1000):
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if cutmix_minmax is not None:
            assert len(cutmix_minmax) == 2
            self.cutmix_alpha = 1.0                              # a min/max box takes no alpha: the reference pins it
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True                                # the training loop may switch mixing off

    # ---- draws, in the reference's order
    def _which(self):
        both = self.mixup_alpha > 0. and self.cutmix_alpha > 0.
        assert both or self.mixup_alpha > 0. or self.cutmix_alpha > 0., \
            "One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true."
        return both

    def _params_per_batch(self):
        """(lam, use_cutmix) for the whole batch.  Draws: rand (apply?), then rand (which?) if both are active, then one beta."""
        if not (self.mixup_enabled and np.random.rand() < self.mix_prob):
            return 1., False
        if self._which():
            cut = np.random.rand() < self.switch_prob
        else:
            cut = not self.mixup_alpha > 0.
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        return float(np.random.beta(alpha, alpha)), cut

    def _params_per_elem(self, batch_size):
        """(lam float32 [n], use_cutmix bool [n]).  Draws: rand(n) (which?) and BOTH betas if both are active, else one beta(n); then rand(n) (apply?)."""
        lam = np.ones(batch_size, dtype=np.float32)
        cut = np.zeros(batch_size, dtype=bool)
        if not self.mixup_enabled:
            return lam, cut
        if self._which():
            cut = np.random.rand(batch_size) < self.switch_prob
            for_cut = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=batch_size)
            for_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=batch_size)
            drawn = np.where(cut, for_cut, for_mix)
        elif self.mixup_alpha > 0.:
            drawn = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=batch_size)
        else:
            cut = np.ones(batch_size, dtype=bool)
            drawn = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=batch_size)
        lam = np.where(np.random.rand(batch_size) < self.mix_prob, drawn.astype(np.float32), lam)
        return lam, cut

    def _draw(self, shape):
        """All of this call's draws -> (shared Record, None) in 'batch' mode, (None, [N Records]) otherwise."""
        if self.mode not in ('elem', 'pair'):
            lam, cut = self._params_per_batch()
            if lam == 1.:
                return UNTOUCHED, None
            box = (0, 0, 0, 0)
            if cut:
                box, lam = cutmix_bbox_and_lam(shape, lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
            return Record(CUTMIX if cut else MIX, np.float32(lam), np.float32(1. - lam), *(int(v) for v in box)), None
        n = shape[0] if self.mode == 'elem' else shape[0] // 2
        lams, cuts = self._params_per_elem(n)
        table = []
        for i in range(n):
            if lams[i] == 1.:
                table.append(UNTOUCHED)
                continue
            box = (0, 0, 0, 0)
            if cuts[i]:
                box, lam = cutmix_bbox_and_lam(shape[1:], lams[i], ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
                lams[i] = lam                                    # rounds the corrected value to fp32
            table.append(Record(CUTMIX if cuts[i] else MIX, lams[i], np.float32(1) - lams[i], *(int(v) for v in box)))
        if self.mode == 'pair':
            table = table + table[::-1]                          # image N-1-i shares image i's parameters
        return None, table

    def __call__(self, x, target):
        global fused_hits
        assert len(x) % 2 == 0, 'Batch size should be even when using this'
        shared, table = self._draw(x.shape)
        if _images_ok(x) and _labels_ok(target, len(x), x.device, self.num_classes):
            staged = _Staged(shared, table, x.device)
            _mix_launch(x, staged)
            fused_hits += 1
            return x, _targets_launch(target, staged, self.num_classes, self.label_smoothing)
        _mix_formula(x, shared, table)
        if shared is not None:
            a, b = float(shared.a), float(shared.b)
        else:                                                    # timm1/data/mixup.py:174, :194: the lam column takes the batch's dtype
            a = torch.tensor(np.array([r.a for r in table], dtype=np.float32), device=x.device, dtype=x.dtype).unsqueeze(1)
            b = 1. - a
        return x, _targets_formula(target, a, b, self.num_classes, self.label_smoothing, x.device)
