"""The fused gradient norm / clipping / loss-scale path without a GPU: argument checks of the four new C entries (nothing is
launched), the state-dict exchange of slak_amd.scaler.NativeScalerWithGradNormCount with torch's GradScaler, and -- where the reference
checkout is present -- its fallback path against the reference's own class."""
import ctypes
import warnings

import pytest
import torch

INVALID = 1                                                          # SLAK_ERR_INVALID_ARG


def test_new_entries_check_their_arguments():
    from slak_amd import _lib, build
    build.build()
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)                            # never dereferenced: the argument checks come first, and no call below launches
    p = ctypes.addressof(buf)
    hyp = (_lib.AdamwGroup * 1)()
    assert L.slak_adamw_plan_blocks(None) == -INVALID                # a count: the error is the one value no count can be
    assert L.slak_grad_sumsq(None, p, None, p, 0, None) == INVALID
    assert L.slak_grad_sumsq(p, None, None, p, 0, None) == INVALID
    assert L.slak_grad_sumsq(p, p, None, None, 0, None) == INVALID
    assert L.slak_grad_sumsq(p, p, None, p, -1, None) == INVALID
    assert L.slak_grad_norm_finish(None, 3, None, -1.0, p, None) == INVALID
    assert L.slak_grad_norm_finish(p, -1, None, -1.0, p, None) == INVALID
    assert L.slak_grad_norm_finish(p, 3, None, 1.0, None, None) == INVALID
    assert L.slak_grad_norm_finish(p, 3, None, float("nan"), p, None) == INVALID
    assert L.slak_adamw_step_scaled(None, p, hyp, 1, p, None) == INVALID
    assert L.slak_adamw_step_scaled(p, None, hyp, 1, p, None) == INVALID
    assert L.slak_adamw_step_scaled(p, p, None, 1, p, None) == INVALID
    assert L.slak_adamw_step_scaled(p, p, hyp, 0, p, None) == INVALID
    assert L.slak_adamw_step_scaled(p, p, hyp, -2, p, None) == INVALID
    assert L.slak_adamw_step_scaled(p, p, hyp, _lib.ADAMW_MAX_GROUPS + 1, p, None) == INVALID
    assert L.slak_adamw_step_scaled(p, p, hyp, 1, None, None) == INVALID
    assert L.slak_version() == 10                                    # no existing entry changed its argument list (10: slak_tri_plan added)


def test_fused_step_has_no_cpu_fallback():
    from slak_amd import _lib
    from slak_amd.optim_factory import MaskedAdamW
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(_lib.SlakHipError):
        MaskedAdamW([p]).step_with_grad_norm(clip_grad=1.0)
    with pytest.raises(ValueError):
        MaskedAdamW([p]).step_with_grad_norm(clip_grad=-1.0)
    assert not hasattr(MaskedAdamW, "_step_supports_amp_scaling")   # GradScaler.step keeps driving step() itself on the reference's AMP branch


def test_state_dict_round_trip():
    """Key for key torch's GradScaler; a GradScaler's state loads and comes back.  (Without a GPU torch disables its GradScaler and both
    state dicts are empty; the GPU suite checks the same with real values.)"""
    from slak_amd.scaler import NativeScalerWithGradNormCount
    assert NativeScalerWithGradNormCount.state_dict_key == "amp_scaler"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours = NativeScalerWithGradNormCount()
        assert ours.state_dict() == torch.cuda.amp.GradScaler().state_dict()
        src = torch.cuda.amp.GradScaler(init_scale=512.0, growth_interval=7)
        ours.load_state_dict(src.state_dict())
        assert ours.state_dict() == src.state_dict()
        again = NativeScalerWithGradNormCount()
        again.load_state_dict(ours.state_dict())
        assert again.state_dict() == ours.state_dict()
        assert NativeScalerWithGradNormCount(enabled=False).state_dict() == {}


@pytest.mark.parametrize("clip_grad", [None, 0.05])
def test_fallback_path_is_the_references_sequence(clip_grad):
    """Any optimizer but MaskedAdamW runs utils.py:390-404 itself: same norm, same parameters as the reference's class, seeded, on the CPU."""
    from oracle import ref_modules
    if not ref_modules.available("reference_utils"):
        pytest.skip("no reference checkout (and no bytecode of its utils.py) here")
    from slak_amd.scaler import NativeScalerWithGradNormCount
    _, utils = ref_modules.load_engine()

    def run(cls):
        torch.manual_seed(0)
        net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
        opt = torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            scaler = cls()
        norms = []
        for _ in range(3):
            opt.zero_grad()
            loss = net(torch.randn(4, 7)).square().sum()
            norms.append(scaler(loss, opt, clip_grad=clip_grad, parameters=net.parameters()))
        assert scaler(net(torch.randn(4, 7)).sum(), opt, update_grad=False) is None
        return norms, [p.detach().clone() for p in net.parameters()], scaler.state_dict()
    (na, pa, sa), (nb, pb, sb) = run(NativeScalerWithGradNormCount), run(utils.NativeScalerWithGradNormCount)
    assert all(torch.equal(a, b) for a, b in zip(na, nb)) and all(torch.equal(a, b) for a, b in zip(pa, pb)) and sa == sb
