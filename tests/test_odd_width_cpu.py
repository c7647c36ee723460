"""Odd / unaligned channel counts (`--width_factor 1.3`: C = 124 / 249 / 499 / 998) -- the host-side part: the NHWC pitch table and the
argument validation of the pitched block-tail entry points (status codes before anything touches a GPU)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from slak_amd import build, _lib
    build.build()
    return _lib.lib()


def test_nhwc_pitch_table():
    from slak_amd import block_ops
    saved = block_ops.pad_even_widths
    try:
        block_ops.pad_even_widths = False
        for C, want in ((96, 96), (128, 128), (768, 768), (16, 16), (4, 4), (124, 124), (998, 998), (249, 256), (499, 512), (5, 64), (1023, 1024),
                        (1025, None)):
            assert block_ops.nhwc_pitch(C) == want, C
        block_ops.pad_even_widths = True
        for C, want in ((96, 96), (124, 128), (998, 1024), (249, 256), (1025, None)):
            assert block_ops.nhwc_pitch(C) == want, C
        for k in range(6):                                   # the standard widths 96 * 2^k and 128 * 2^k are never padded
            for base in (96, 128):
                C = base << k
                assert block_ops.nhwc_pitch(C) == (C if C <= 1024 else None)
    finally:
        block_ops.pad_even_widths = saved


def test_pad_even_widths_is_off_by_default():
    import os
    from slak_amd import block_ops
    assert block_ops.pad_even_widths == (os.environ.get("SLAK_PAD_EVEN", "0") == "1")


@pytest.mark.parametrize("C,ldc", [(249, 248), (249, 252), (249, 250), (1023, 1032), (999, 2048), (124, 120), (64, 68)])
def test_pitched_entry_points_refuse_bad_pitches(L, C, ldc):
    """ldc < C, ldc % 8 != 0, ldc > 1024 -> SLAK_ERR_UNSUPPORTED from all four entry points (decided on the host, before any launch)."""
    from slak_amd import _lib
    buf = ctypes.create_string_buffer(64)                    # never dereferenced: the shape check comes first
    p = ctypes.cast(buf, ctypes.c_void_p)
    N, P = 2, 49
    assert L.slak_ln_nchw_to_nhwc_forward_ld(p, p, p, p, p, p, N, C, P, 1e-6, None, ldc) == _lib.ERR_UNSUPPORTED
    assert L.slak_ln_nchw_to_nhwc_backward_ld(p, p, p, p, p, p, p, p, N, C, P, p, 1 << 30, None, ldc) == _lib.ERR_UNSUPPORTED
    assert L.slak_scale_residual_forward_ld(p, _lib.SLAK_F32, p, p, None, p, None, N, C, P, None, ldc) == _lib.ERR_UNSUPPORTED
    assert L.slak_scale_residual_backward_ld(p, None, None, p, p, None, p, p, p, N, C, P, p, 1 << 30, None, ldc) == _lib.ERR_UNSUPPORTED


# C = 98: the family query answers TILE for ldc == C, so the pitched call must get as far as the workspace check; 249, 5: ldc == C needs an even C;
# 96, 1024: multiples of 8, which both rules always took; 1026: above the limit
@pytest.mark.parametrize("C,P,want", [(98, 400, 3), (249, 49, 2), (5, 9, 2), (96, 196, 3), (1024, 49, 3), (1026, 49, 2)])
def test_pitch_equal_to_c_gets_the_status_of_the_plain_entry_point(L, C, P, want):
    """One argument rule: with ldc == C the four `_ld` entry points return what the plain ones return (want: 3 = SLAK_ERR_WORKSPACE behind an
    accepted shape, 2 = SLAK_ERR_UNSUPPORTED), and the family query agrees.  Host code only: a 16-byte workspace stops every accepted call."""
    from slak_amd import _lib
    assert want in (3, _lib.ERR_UNSUPPORTED)
    buf = ctypes.create_string_buffer(64)                    # never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    N = 2
    bwd = ((L.slak_ln_nchw_to_nhwc_backward, L.slak_ln_nchw_to_nhwc_backward_ld, (p, p, p, p, p, p, p, p, N, C, P, p, 16, None)),
           (L.slak_scale_residual_backward, L.slak_scale_residual_backward_ld, (p, None, None, p, p, None, p, p, p, N, C, P, p, 16, None)))
    for plain, ld, args in bwd:
        assert plain(*args) == want and ld(*args, C) == want
    # the forward ops have no workspace: only a refusal can be asked for without a device (an unknown shortcut dtype refuses an accepted shape)
    if want == _lib.ERR_UNSUPPORTED:
        assert L.slak_ln_nchw_to_nhwc_forward(p, p, p, p, p, p, N, C, P, 1e-6, None) == want
        assert L.slak_ln_nchw_to_nhwc_forward_ld(p, p, p, p, p, p, N, C, P, 1e-6, None, C) == want
    for sdt in ((_lib.SLAK_F32, 99) if want == _lib.ERR_UNSUPPORTED else (99,)):
        assert L.slak_scale_residual_forward(p, sdt, p, p, None, p, None, N, C, P, None) == _lib.ERR_UNSUPPORTED
        assert L.slak_scale_residual_forward_ld(p, sdt, p, p, None, p, None, N, C, P, None, C) == _lib.ERR_UNSUPPORTED
    for op in range(4):
        assert (L.slak_block_tail_family(op, _lib.SLAK_F32, N, C, P, C) != 0) == (want == 3)


def test_pitched_entry_points_check_pointers_and_workspace(L):
    from slak_amd import _lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.slak_ln_nchw_to_nhwc_forward_ld(None, p, p, p, p, p, 2, 249, 49, 1e-6, None, 256) == _lib.ERR_INVALID_ARG
    assert L.slak_scale_residual_forward_ld(p, _lib.SLAK_F32, p, p, None, p, None, 0, 249, 49, None, 256) == _lib.ERR_INVALID_ARG
    assert L.slak_ln_nchw_to_nhwc_backward_ld(p, p, p, p, p, p, p, p, 2, 249, 49, p, 16, None, 256) == 3          # SLAK_ERR_WORKSPACE
    assert L.slak_scale_residual_backward_ld(p, None, None, p, p, None, p, p, p, 2, 249, 49, None, 0, None, 256) == 3
    assert L.slak_pad_cast_bf16_batch(None, None, None, None, None, None, None, 0, None) == _lib.OK                # nothing to do
    assert L.slak_pad_cast_bf16_batch(None, None, None, None, None, None, None, 1, None) == _lib.ERR_INVALID_ARG
