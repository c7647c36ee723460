"""slak_block_tail_family: which kernel family a block-tail entry point runs (no GPU needed: host code).

The pitched entry points (`slak_*_ld`) take the small-plane families -- `chan` (even planes of at most 256 pixels, a wave per image and channel
group) and `chan1` (odd planes, one pixel per lane) -- where the plain entry point on C = ldc takes them, ahead of the pixel-pair register-tile
kernels; everything else keeps the family it had.  The entry points branch on this very function, so what it answers is what is launched.
"""
import itertools

import pytest

LN_FWD, LN_BWD, SR_FWD, SR_BWD = 0, 1, 2, 3
NONE, TILE, REG, CHAN, CHAN1 = 0, 1, 2, 3, 4
OPS = (LN_FWD, LN_BWD, SR_FWD, SR_BWD)


@pytest.fixture(scope="module")
def fam():
    from slak_amd import _lib
    L = _lib.lib()
    assert (_lib.TAIL_LN_FWD, _lib.TAIL_LN_BWD, _lib.TAIL_SR_FWD, _lib.TAIL_SR_BWD) == OPS
    assert (_lib.TAIL_FAMILY_NONE, _lib.TAIL_FAMILY_TILE, _lib.TAIL_FAMILY_REG, _lib.TAIL_FAMILY_CHAN, _lib.TAIL_FAMILY_CHAN1) == (NONE, TILE, REG, CHAN, CHAN1)
    f32 = _lib.SLAK_F32

    def f(op, N, C, P, ldc, dt=f32):
        return int(L.slak_block_tail_family(op, dt, N, C, P, ldc))
    return f


@pytest.mark.parametrize("N,C,P,ldc", [(128, 499, 196, 512), (2, 249, 196, 256)])
def test_even_small_planes_take_chan(fam, N, C, P, ldc):
    for op in (SR_FWD, SR_BWD, LN_BWD):
        assert fam(op, N, C, P, ldc) == CHAN, op
    assert fam(LN_FWD, N, C, P, ldc) == REG         # the forward LayerNorm has no `chan` kernel (it measured slower and was dropped)


@pytest.mark.parametrize("N,C,P,ldc", [(128, 998, 49, 1024), (128, 499, 49, 512), (2, 249, 49, 256)])
def test_odd_small_planes_take_chan1(fam, N, C, P, ldc):
    for op in OPS:
        assert fam(op, N, C, P, ldc) == CHAN1, op


def test_nothing_changes_elsewhere(fam):
    from slak_amd import _lib
    for op in OPS:
        assert fam(op, 128, 249, 784, 256) == REG, op               # 28 x 28: the pixel-pair `LD` kernels
        assert fam(op, 2, 5, 9, 64) == fam(op, 2, 64, 9, 64), op    # tiny C on a pitch: what the plain C = 64 call runs
    # SLaK-B's stage 3 on a pitch of 704: no pixel-pair instantiation, and eleven groups of 64 are more than the eight waves of the LayerNorm
    # `chan` kernel -> the LDS-tile kernels, as before.  (The two residual ops have no wave limit: the plain call on C = 704 runs `chan` with
    # 64 / 32 channels per wave, so by the rule above the pitched call does too.)
    for op in (LN_FWD, LN_BWD):
        assert fam(op, 128, 665, 196, 704) == TILE, op
    for op in (SR_FWD, SR_BWD):
        assert fam(op, 128, 665, 196, 704) == fam(op, 128, 704, 196, 704) == CHAN, op
    assert fam(SR_FWD, 128, 499, 196, 512, _lib.SLAK_BF16) == REG   # a bf16 shortcut has no small-plane family
    assert fam(SR_FWD, 128, 499, 49, 512, _lib.SLAK_BF16) == TILE
    assert fam(SR_FWD, 128, 499, 196, 512, _lib.SLAK_F16) == NONE
    assert fam(LN_FWD, 128, 499, 196, 510) == NONE and fam(LN_FWD, 128, 1025, 196, 1032) == NONE and fam(7, 2, 64, 9, 64) == NONE


GRID_N = (1, 2, 128, 8193)
GRID_P = (1, 2, 9, 49, 64, 196, 255, 256, 258, 784)
GRID_LDC = (64, 96, 128, 192, 256, 384, 512, 704, 768, 1024)


def test_pitched_answer_is_the_plain_answer_where_that_is_a_small_plane_family(fam):
    seen = set()
    for op, N, P, ldc, pad in itertools.product(OPS, GRID_N, GRID_P, GRID_LDC, (1, 7, 13, 40, 63)):
        plain = fam(op, N, ldc, P, ldc)
        got = fam(op, N, ldc - pad, P, ldc)
        assert (got == NONE) == (plain == NONE), (op, N, P, ldc, pad)      # (N * ldc * P past 2^31: the same limit on both)
        if plain == NONE:
            continue
        if plain in (CHAN, CHAN1):
            assert got == plain, (op, N, P, ldc, pad, got, plain)
            seen.add((op, plain))
        elif got in (CHAN, CHAN1):
            # the one rung the pitched calls have of their own: the LayerNorm kernels on odd planes with 64 channels per wave where the plain
            # instantiations (48 / 32 per wave) would need more than 16 waves
            assert op in (LN_FWD, LN_BWD) and got == CHAN1 and P % 2 == 1 and ldc % 64 == 0 and ldc // 32 > 16 and ldc % 48 != 0, (op, N, P, ldc, pad)
        if plain == TILE and not (got == CHAN1 and op in (LN_FWD, LN_BWD)):
            assert got == TILE, (op, N, P, ldc, pad)
        if got == REG:
            assert plain == REG and pad <= 16 and P % 2 == 0, (op, N, P, ldc, pad)
    assert seen == {(LN_BWD, CHAN), (SR_FWD, CHAN), (SR_BWD, CHAN)} | {(op, CHAN1) for op in OPS}


def test_pitch_equal_to_c_is_the_plain_choice(fam):
    # the plain ladder: small planes, then the pixel-pair kernels where C has an instantiation, then the LDS-tile kernels
    assert [fam(op, 128, 384, 196, 384) for op in OPS] == [REG, CHAN, CHAN, CHAN]
    assert [fam(op, 128, 768, 49, 768) for op in OPS] == [CHAN1] * 4
    assert [fam(op, 128, 1024, 49, 1024) for op in OPS] == [TILE, TILE, CHAN1, CHAN1]
    assert [fam(op, 128, 96, 3136, 96) for op in OPS] == [REG] * 4
    assert [fam(op, 128, 320, 3136, 320) for op in OPS] == [TILE] * 4
    assert [fam(op, 128, 97, 196, 97) for op in OPS] == [NONE] * 4          # the plain entry points want an even C
