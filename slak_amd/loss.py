"""The criterion of the training step on one HIP launch per direction (slak_xent_forward / slak_xent_backward, csrc/xent.hip).

The reference picks its criterion at main.py:398-403: ``SoftTargetCrossEntropy`` when mixup is on (every README recipe), else
``LabelSmoothingCrossEntropy(smoothing)`` when smoothing > 0, else ``torch.nn.CrossEntropyLoss``.  The three classes here carry the same
names, constructor arguments and results (timm1/loss/cross_entropy.py:11-26 and :29-36); ``cross_entropy`` is the functional form
they share.  Where the kernel does not apply -- CPU tensors, arguments it does not take -- the same formula runs as torch ops in float32:
the result never depends silently on which path ran, and ``fused_hits`` counts the calls the kernel served.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

__all__ = ["cross_entropy", "CrossEntropyLoss", "LabelSmoothingCrossEntropy", "SoftTargetCrossEntropy"]

fused_hits = 0                # forwards the HIP kernel served so far (tests, tools/time_width.py)
_NO_LABEL = -2 ** 63          # an ignore_index no label equals: the timm formulas ignore nothing
_DT = {torch.float32: _lib.SLAK_F32, torch.float16: _lib.SLAK_F16, torch.bfloat16: _lib.SLAK_BF16}


def _torch_formula(logits, target, label_smoothing, ignore_index):
    """The formulas of include/slak_hip.h (slak_xent_*) as torch ops on float32 log-probabilities; float32 result."""
    lp = F.log_softmax(logits.float(), dim=-1)
    K = logits.shape[-1]
    if target.is_floating_point():                               # sum_k -t_k log p_k, mean over the rows (timm1/loss/cross_entropy.py:34-36)
        t = target.float()
        if label_smoothing > 0.0:                                # torch's rule for probability targets
            t = t * (1.0 - label_smoothing) + label_smoothing / K
        return -(t * lp).sum(-1).mean()
    counts = target != ignore_index
    picked = lp.gather(-1, torch.where(counts, target, torch.zeros_like(target)).unsqueeze(-1)).squeeze(-1)
    per_row = -(1.0 - label_smoothing) * picked - label_smoothing * lp.mean(-1)     # timm1/loss/cross_entropy.py:20-26
    return torch.where(counts, per_row, torch.zeros_like(per_row)).sum() / counts.sum().to(per_row.dtype)


def _fused_ok(logits, target, label_smoothing):
    if not (logits.is_cuda and logits.dim() == 2 and logits.dtype in _DT and target.device == logits.device and 0.0 <= label_smoothing < 1.0):
        return False
    N, K = logits.shape
    if N < 1 or K < 1:
        return False
    if target.is_floating_point():
        if target.shape != logits.shape or label_smoothing != 0.0 or target.requires_grad:
            return False
    elif target.dtype != torch.int64 or target.shape != (N,):
        return False
    return bool(_lib.lib().slak_xent_supported(_DT[logits.dtype], N, K))


class _Xent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, label_smoothing, ignore_index):
        global fused_hits
        from .ops import _workspace, _stream, _on
        if logits.stride(1) != 1 or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
            logits = logits.contiguous()                         # rows must be contiguous; a row stride is passed on
        N, K = logits.shape
        soft = target.is_floating_point()
        target = target.to(torch.float32).contiguous() if soft else target.contiguous()
        dev = logits.device
        loss = torch.empty((), dtype=torch.float32, device=dev)  # a tensor of its own: engine.py:79 divides the loss in place, which autograd refuses on a view
        count = torch.empty(1, dtype=torch.float32, device=dev)
        lse = torch.empty(N, dtype=torch.float32, device=dev)
        L = _lib.lib()
        ws, nb = _workspace(L.slak_xent_workspace_bytes(N, K), dev)
        with _on(dev):
            _lib.check(L.slak_xent_forward(logits.data_ptr(), _DT[logits.dtype], logits.stride(0), None if soft else target.data_ptr(),
                                           target.data_ptr() if soft else None, float(label_smoothing), int(ignore_index),
                                           loss.data_ptr(), lse.data_ptr(), count.data_ptr(), N, K,
                                           ws.data_ptr() if ws is not None else None, nb, _stream(dev)), "slak_xent_forward")
        ctx.save_for_backward(logits, target, lse, count)
        ctx.args = (soft, float(label_smoothing), int(ignore_index))
        fused_hits += 1
        return loss

    @staticmethod
    def backward(ctx, g):
        from .ops import _stream, _on
        logits, target, lse, count = ctx.saved_tensors
        soft, smoothing, ignore_index = ctx.args
        N, K = logits.shape
        dev = logits.device
        g = g.to(torch.float32).contiguous()                     # a device scalar: it is never read on the host
        d = torch.empty((N, K), dtype=logits.dtype, device=dev)
        with _on(dev):
            _lib.check(_lib.lib().slak_xent_backward(logits.data_ptr(), _DT[logits.dtype], logits.stride(0), None if soft else target.data_ptr(),
                                                     target.data_ptr() if soft else None, smoothing, ignore_index, lse.data_ptr(),
                                                     count.data_ptr(), g.data_ptr(), d.data_ptr(), N, K, _stream(dev)), "slak_xent_backward")
        return d, None, None, None


def cross_entropy(logits, target, label_smoothing=0.0, ignore_index=-100):
    """Mean cross-entropy of ``logits`` (N, K) against ``target``: int64 class indices (N,) -- == ``F.cross_entropy(logits, target,
    label_smoothing=..., ignore_index=...)`` -- or floating probabilities (N, K) -- == ``torch.sum(-target * log_softmax(logits), -1).mean()``.

    ONE autograd node on one launch per direction for float32 / bfloat16 / float16 CUDA logits.  Returns a float32 0-dim loss WHATEVER the
    logits' dtype (the arithmetic is float32; under autocast that is torch's own result dtype, outside autocast torch would round the loss of
    bfloat16 logits to bfloat16).  Anything the kernel does not take runs the same formula as torch ops in float32."""
    label_smoothing = float(label_smoothing)
    if _fused_ok(logits, target, label_smoothing):
        return _Xent.apply(logits, target, label_smoothing, int(ignore_index))
    return _torch_formula(logits, target, label_smoothing, int(ignore_index))


class CrossEntropyLoss(nn.CrossEntropyLoss):
    """``torch.nn.CrossEntropyLoss`` (main.py:403) on the fused op; with class weights or another reduction than 'mean': torch's own op."""

    def forward(self, input, target):
        if self.weight is None and self.reduction == "mean":
            return cross_entropy(input, target, self.label_smoothing, self.ignore_index)
        return super().forward(input, target)


class LabelSmoothingCrossEntropy(nn.Module):
    """timm1/loss/cross_entropy.py:11-26 (main.py:401): (1 - smoothing) * nll + smoothing * mean_k(-log p_k), mean over the rows."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1.0 - smoothing

    def forward(self, x, target):
        return cross_entropy(x, target, self.smoothing, _NO_LABEL)


class SoftTargetCrossEntropy(nn.Module):
    """timm1/loss/cross_entropy.py:29-36 (main.py:399): sum_k -t_k log p_k, mean over the rows; ``target`` is mixup's (N, K) distribution."""

    def forward(self, x, target):
        return cross_entropy(x, target, 0.0, _NO_LABEL)
