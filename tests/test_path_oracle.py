"""CPU: the properties of tests/path_oracle.py, the fp64 definition of fftup_shift_path the driver and the kernel are held to."""
import numpy as np

import path_oracle as PO


def _rows(pairs, peak=1.0):
    return np.array([[dx, dy, peak, peak] for dx, dy in pairs], np.float32)


def test_a_constant_increment_gets_no_offset_away_from_the_ends():
    """p linear: the symmetric window's mean is p itself wherever the window is not clamped -- |out| <= 1e-12 for r <= i < n - r
    (seen: 1e-13); at the clip's ends the clamped window lags, by 1.18 px here"""
    n, sigma = 200, 4.0
    r = 12
    for mode, rows in ((PO.CONSECUTIVE, _rows([(0.75, -0.5)] * n)), (PO.ABSOLUTE, _rows([(0.75 * i, -0.5 * i) for i in range(n)]))):
        p, s, out = PO.path(rows, mode, sigma)
        assert np.array_equal(p[:, 0], 0.75 * np.arange(n)) and np.array_equal(p[:, 1], -0.5 * np.arange(n))
        assert np.abs(out[r:n - r]).max() <= 1e-12
        assert abs(out[0, 0]) > 1.0 and abs(out[-1, 0]) > 1.0 and abs(out[0, 1]) > 0.5
        print("MEASURED path_oracle linear mode %d: interior %.3g ends %.3g" % (mode, np.abs(out[r:n - r]).max(), np.abs(out[[0, -1]]).max()))


def test_sigma_zero_absolute_returns_the_input():
    sh = _rows([(1.25, -3.5), (0.0, 7.0), (-2.0, 0.125)])
    got = PO.offsets(sh, PO.ABSOLUTE, 0.0)
    assert got.tobytes() == sh.tobytes()
    p, s, out = PO.path(sh, PO.ABSOLUTE, 0.0)
    assert not s.any() and np.array_equal(out, sh[:, :2].astype(np.float64))


def test_unmeasured_frames_hold_the_path():
    sh = _rows([(1, 1), (5, 5), (2, 2)])
    sh[1, 2] = 0.1                              # below min_peak
    p, _, out = PO.path(sh, PO.ABSOLUTE, 0.0, 0.5)
    assert out.tolist() == [[1, 1], [1, 1], [2, 2]]
    p, _, out = PO.path(sh, PO.CONSECUTIVE, 0.0, 0.5)
    assert out.tolist() == [[0, 0], [0, 0], [2, 2]]        # in[0] ignored, frame 1 adds nothing
    p, _, out = PO.path(sh, PO.CONSECUTIVE, 0.0, 0.0)
    assert out.tolist() == [[0, 0], [5, 5], [7, 7]]
    # a NaN peak, a NaN dx and an infinite dy all make a frame unmeasured, both axes at once
    for col, bad in ((2, np.nan), (0, np.nan), (1, np.inf)):
        t = _rows([(1, 1), (5, 5), (2, 2)])
        t[1, col] = bad
        assert PO.path(t, PO.ABSOLUTE, 0.0)[0].tolist() == [[1, 1], [1, 1], [2, 2]]
        assert PO.path(t, PO.CONSECUTIVE, 0.0)[0].tolist() == [[0, 0], [0, 0], [2, 2]]
    # ... and ahead of the first measured frame the path is 0
    t = _rows([(3, 3), (4, 4)])
    t[0, 2] = np.nan
    assert PO.path(t, PO.ABSOLUTE, 0.0)[0].tolist() == [[0, 0], [4, 4]]


def test_one_frame_gives_zero():
    for mode in PO.MODES:
        for sigma in (0.0, 1.5, 256.0):
            p, s, out = PO.path(_rows([(3.5, -2.0)]), mode, sigma)
            if mode == PO.CONSECUTIVE:
                assert not out.any()                            # p[0] = 0 whatever in[0] holds
            elif sigma > 0:
                assert np.abs(out).max() <= 1e-12               # the window is frame 0 alone: s = (sum g p) / (sum g), p up to rounding
            else:
                assert out.tolist() == [[3.5, -2.0]]            # (ABSOLUTE, sigma 0: locked on the reference)


def test_a_window_wider_than_the_clip_is_the_clamped_sum():
    sigma, r = 8.0, 24
    p, s, out = PO.path(_rows([(1.0, 2.0), (3.0, -4.0)]), PO.ABSOLUTE, sigma)
    g = np.exp(-np.arange(-r, r + 1) ** 2 / (2 * sigma * sigma))
    for i in (0, 1):
        w1 = g[np.arange(-r, r + 1) + i >= 1].sum() / g.sum()           # the weight that lands on frame 1 (clamped from above)
        for a in (0, 1):
            assert abs(s[i, a] - ((1 - w1) * p[0, a] + w1 * p[1, a])) <= 1e-14
    assert 0.5 < (s[1, 0] - 1.0) / 2.0 < 0.6 and 0.4 < (s[0, 0] - 1.0) / 2.0 < 0.5


def test_offsets_copy_the_peaks_and_round_once():
    sh = PO.grid_shifts(65, 5)
    got = PO.offsets(sh, PO.CONSECUTIVE, 1.5, 0.5)
    assert got[:, 2:].tobytes() == sh[:, 2:].tobytes() and got.dtype == np.float32
    assert np.array_equal(got[:, :2], PO.path(sh, PO.CONSECUTIVE, 1.5, 0.5)[2].astype(np.float32))
    assert np.isfinite(got[:, :2]).all()


def test_the_grid_is_the_issue_s():
    assert len(PO.GRID) == 29 and (4096, 64.0) in PO.GRID and (7, 256.0) in PO.GRID and (65, 0.4) in PO.GRID
    sh, (p, s, out) = PO.grid_case(65, 1.5, PO.ABSOLUTE, 0.5)
    assert np.isnan(sh[:, 0]).sum() == 1 and np.isinf(sh[:, :2]).sum() == 2 and np.isnan(sh[:, 2]).sum() == 1
    assert np.isfinite(out).all() and PO.grid_case(65, 1.5, PO.ABSOLUTE, 0.5)[0] is sh
