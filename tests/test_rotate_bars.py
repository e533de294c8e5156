"""CPU: where the fp32 bars of tests/test_gpu_rotate.py come from (tests/rotate_cases.py): the oracle run in complex64 against the
oracle run in complex128 over exactly the GPU tests' frames.  The recorded figures C64_MAX_ABS and C64_REL_L2 must be what this
measures -- not below it, and not more than twice it, so that a bar cannot drift away from its derivation -- and the oracle's share
of near-ties of the 8-bit store must stay under the cap the GPU test asserts."""
import numpy as np
import pytest

import paritylib as P
import rotate_cases as K
import rotate_oracle as R


@pytest.fixture(scope="module")
def figures():
    rows = []
    for (W, H) in R.CASES:
        for kind in ("u8", "f32", "f16"):
            d, s = K.oracle(W, H, kind), K.oracle(W, H, kind, single=True)
            rows.append((W, H, kind, max(float(np.abs(x - y).max()) for x, y in zip(d, s)), max(P.rel_l2(y, x) for x, y in zip(d, s)),
                         max(float(K.near_tie(x).mean()) for x in d)))
            print("MEASURED rotate complex64 oracle %dx%d %s: max|diff| %.3g  rel L2 %.3g  near-tie share %.3g" % rows[-1])
    return rows


def test_recorded_figures_are_the_measured_ones(figures):
    mx, l2 = max(r[3] for r in figures), max(r[4] for r in figures)
    assert 0.5 * K.C64_MAX_ABS <= mx <= K.C64_MAX_ABS, mx
    assert 0.5 * K.C64_REL_L2 <= l2 <= K.C64_REL_L2, l2
    assert K.FP32_ABS == 4 * K.C64_MAX_ABS and K.FP32_REL_L2 == 4 * K.C64_REL_L2


def test_near_ties_of_the_oracle_stay_under_the_cap(figures):
    """with 8-bit uniform noise 2 * 255 * FP32_ABS = 1.3e-3 of a frame is expected within 255 FP32_ABS of a rounding tie, and at
    most 2.3e-3 is measured (64 x 32, the smallest frame); the cap is 1 %, four times what is allowed here"""
    assert max(r[5] for r in figures) <= K.NEAR_TIE_CAP / 4


def test_seven_frames_and_every_angle():
    for (W, H) in R.CASES:
        rots = K.rotations(W, H)
        assert len(rots) == K.N_FRAMES == 7 and [r[0] for r in rots[:5]] == R.ANGLES
        assert rots[5][1:] != R.centre_of(W, H) and all(abs(r[0]) <= np.pi / 2 for r in rots)
