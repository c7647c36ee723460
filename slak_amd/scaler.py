"""``NativeScalerWithGradNormCount`` of the reference (utils.py:384-410) with the gradient norm, the clipping, the found-inf test
and the optimizer step on ``2 * plans + 1`` HIP launches and no host synchronisation.

The reference's ``__call__`` runs, per update: ``GradScaler.unscale_`` (a read-and-write pass over every gradient, then ``.item()``
on found_inf inside ``GradScaler.step``), ``get_grad_norm_`` (utils.py:413-425: one ``torch.norm`` per parameter, a ``stack`` and
another ``norm``) or ``clip_grad_norm_`` (one more read-and-write pass), ``scaler.step(optimizer)``, ``scaler.update()``.
With a :class:`slak_amd.optim_factory.MaskedAdamW` this class replaces all of it by ``optimizer.step_with_grad_norm`` and one
``torch._amp_update_scale_`` fed with the device found-inf flag.  With any other optimizer, or ``create_graph=True``, it runs the
reference's own sequence on the same ``torch.amp.GradScaler``, so it can stand in everywhere ``utils.NativeScalerWithGradNormCount``
is constructed (main.py:383).

One observable difference from the reference, on the fused path only: ``p.grad`` keeps the SCALED, UNCLIPPED values after the call
(the kernels read the gradients and never write them); the reference leaves them unscaled and clipped.  The returned norm, the
parameters, the optimizer state and the scale trajectory are the reference's.  On the fused path the norm is over the optimizer's
parameters (``parameters`` is not consulted), and with ``enabled=False`` a step whose gradients hold an inf or NaN is skipped.
"""
import torch

from .optim_factory import MaskedAdamW

__all__ = ["NativeScalerWithGradNormCount", "get_grad_norm_"]


def get_grad_norm_(parameters, norm_type: float = 2.0) -> torch.Tensor:
    """utils.py:413-425 (the fallback path's norm when no clipping is asked for)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = [p for p in parameters if p.grad is not None]
    norm_type = float(norm_type)
    if len(parameters) == 0:
        return torch.tensor(0.)
    device = parameters[0].grad.device
    if norm_type == float("inf"):
        return max(p.grad.detach().abs().max().to(device) for p in parameters)
    return torch.norm(torch.stack([torch.norm(p.grad.detach(), norm_type).to(device) for p in parameters]), norm_type)


class NativeScalerWithGradNormCount:
    """utils.py:384-410.  The scale and the growth tracker are the device tensors of one ``torch.amp.GradScaler`` (2^16, growth 2.0,
    backoff 0.5 every 2000 clean steps, as the reference's default construction), shared by the fused and the fallback path;
    ``state_dict()`` / ``load_state_dict()`` are that GradScaler's, so a reference checkpoint's ``scaler`` entry loads and vice versa.
    ``enabled=False`` is for bf16, which needs no loss scaling: the scale is 1 and never updated, the call still yields the norm,
    the clipping and the step."""

    state_dict_key = "amp_scaler"

    def __init__(self, enabled=True, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self._scaler = torch.amp.GradScaler("cuda", init_scale=init_scale, growth_factor=growth_factor, backoff_factor=backoff_factor,
                                            growth_interval=growth_interval, enabled=enabled)

    def __call__(self, loss, optimizer, clip_grad=None, parameters=None, create_graph=False, update_grad=True):
        self._scaler.scale(loss).backward(create_graph=create_graph)
        if not update_grad:
            return None
        if isinstance(optimizer, MaskedAdamW) and not create_graph:
            return self._fused_update(optimizer, clip_grad)
        if clip_grad is not None:                                   # the reference's own sequence, utils.py:393-401
            assert parameters is not None
            self._scaler.unscale_(optimizer)
            norm = torch.nn.utils.clip_grad_norm_(parameters, clip_grad)
        else:
            self._scaler.unscale_(optimizer)
            norm = get_grad_norm_(parameters)
        self._scaler.step(optimizer)
        self._scaler.update()
        return norm

    def _fused_update(self, optimizer, clip_grad):
        s = self._scaler
        if not s.is_enabled():
            return optimizer.step_with_grad_norm(clip_grad=clip_grad, inv_scale=None)
        scale, tracker = s._scale, s._growth_tracker                # created on the loss's device by scale(loss) above
        inv_scale = scale.double().reciprocal().float()             # as GradScaler._unscale_grads_ forms it
        norm = optimizer.step_with_grad_norm(clip_grad=clip_grad, inv_scale=inv_scale)
        found_inf = optimizer.last_grad_control[2:3]
        # GradScaler.update() without the host: halve on overflow, double after growth_interval clean steps
        torch._amp_update_scale_(scale, tracker, found_inf, s.get_growth_factor(), s.get_backoff_factor(), s.get_growth_interval())
        return norm

    def state_dict(self):
        return self._scaler.state_dict()

    def load_state_dict(self, state_dict):
        self._scaler.load_state_dict(state_dict)
