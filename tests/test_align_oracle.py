"""CPU: the fp64 restatement of the shift estimate (tests/align_oracle.py) against shifts that are known -- the yardstick of
tests/test_gpu_align.py has to be right itself, sign convention included: cur(x, y) ~ ref(x - dx, y - dy).

The bars are conditions on the method, not tuned to it: a quarter of a window pixel on the 64 x 32 windows (8-bit frames, a window
that sees another crop of the scene after the move), a twentieth on 128 x 64, and a peak of at least 0.5."""
import numpy as np
import pytest

import align_oracle as AO

BAR = {(64, 32): 0.25, (128, 64): 0.05}


@pytest.mark.parametrize("case", AO.CASES, ids=["%dx%d_w%dx%d_d%d" % (c[0], c[1], c[2][0], c[2][1], c[3]) for c in AO.CASES])
def test_oracle_recovers_known_shifts(case):
    W, H, window, d = case
    g = AO.geometry(W, H, window, d)
    ref, moved, true = AO.case_clip(W, H, d)
    worst, low = 0.0, 1.0
    for cur, (tx, ty) in zip(moved, true):
        e = AO.estimate(ref, cur, g)
        err = max(abs(e["dx"] - tx), abs(e["dy"] - ty)) / d
        print("MEASURED %dx%d d=%d shift (%.2f, %.2f): got (%.3f, %.3f) err %.3f window px, peak %.3f coarse %.3f gap %.3g"
              % (W, H, d, tx, ty, e["dx"], e["dy"], err, e["peak"], e["peak_coarse"], e["gap"]))
        worst, low = max(worst, err), min(low, e["peak"])
        assert err <= BAR[window], (tx, ty, e)
        assert e["peak"] >= 0.5, e
    print("MEASURED %dx%d d=%d: worst error %.3f window px, lowest peak %.3f" % (W, H, d, worst, low))


def test_sign_convention_and_identical_frames():
    """a frame moved right and down by whole pixels gives positive dx and dy; a frame against itself gives exactly zero and peak 1"""
    W, H, window, d = AO.CASES[0]
    g = AO.geometry(W, H, window, d)
    ref, cur = AO.clip(W, H, d, [(0.0, 0.0), (2.0, 1.0)], seed=3)
    assert np.array_equal(cur[1:, 2:], ref[:-1, :-2]) or np.abs(cur[1:, 2:].astype(int) - ref[:-1, :-2].astype(int)).max() <= 1
    e = AO.estimate(ref, cur, g)
    assert abs(e["dx"] - 2.0) <= 0.25 and abs(e["dy"] - 1.0) <= 0.25 and e["coarse"] == (2, 1), e
    same = AO.estimate(ref, ref, g)
    assert same["dx"] == 0.0 and same["dy"] == 0.0 and abs(same["peak"] - 1.0) < 1e-12 and abs(same["peak_coarse"] - 1.0) < 1e-12, same


def test_geometry_examples():
    for (W, H), want in (((1920, 1080), (1, 1024, 1024)), ((3840, 2160), (2, 1024, 1024)), ((80, 48), (1, 64, 32))):
        g = AO.geometry(W, H)
        assert (g["d"], g["nx"], g["ny"]) == want, g
    g = AO.geometry(600, 300, (512, 256))
    assert (g["crop_x"], g["crop_y"], g["band_kx"], g["band_ky"], g["kappa"]) == (44, 22, 128, 64, 32)
