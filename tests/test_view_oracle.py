"""CPU: the fp64 statement of the view plans (tests/view_oracle.py) against what is already known -- the exact-size oracle on the
full-frame lattices, and the properties a trigonometric interpolant has.  Everything to 1e-12."""
import numpy as np
import pytest

import exactsize_oracle as E
import view_oracle as V

# fold, split, kept Nyquist bin and both parities
PAIRS = [(50, 32), (40, 25), (64, 64), (45, 64), (46, 70), (21, 21), (32, 50), (30, 48)]
TOL = 1e-12


@pytest.mark.parametrize("align", [E.ALIGN_CORNER, E.ALIGN_CENTRE])
@pytest.mark.parametrize("N,M", PAIRS)
def test_full_frame_lattice_is_the_exactsize_rule(N, M, align):
    """origin = delta, span = N: the amplitude-preserving exact-size map, resample_matrix M / N"""
    want = E.resample_matrix(N, M, align) * M / N
    got = V.view_matrix(N, M, E.delta(N, M, align), N)
    assert np.abs(got - want).max() <= TOL


@pytest.mark.parametrize("N,M,origin,span", [(48, 40, 10.3, 17.9), (45, 64, -3.25, 61.5), (50, 32, 5.5, 77.7), (46, 70, 0.4, 23.0),
                                             (21, 30, 2.5, 33.3), (40, 36, 7.75, 12.2), (32, 20, 0.0, 40.0), (4096, 16, 0.5, 16.0)])
def test_real_constant_and_chirp(N, M, origin, span):
    Vm = V.view_matrix(N, M, origin, span)
    assert np.abs(Vm.imag).max() <= TOL                                 # the map is real
    assert np.abs(Vm.sum(axis=1) - 1.0).max() <= TOL                    # constants stay constant
    x = np.random.default_rng(N + M).random(N)
    assert np.abs(V.view_1d_chirp(x, M, origin, span) - V.view_1d(x, M, origin, span)).max() <= TOL   # the chirp-z factorisation


@pytest.mark.parametrize("N,M,origin,span", [(48, 40, 10.3, 17.9), (45, 64, -3.25, 61.5), (50, 32, 5.5, 77.7)])
def test_moving_the_origin_is_rolling_the_input(N, M, origin, span):
    x = np.random.default_rng(3).random(N)
    a = V.view_1d(x, M, origin + 3, span)
    b = V.view_1d(np.roll(x, -3), M, origin, span)
    assert np.abs(a - b).max() <= TOL
    # and the frame is periodic: a whole period changes nothing
    assert np.abs(V.view_1d(x, M, origin + N, span) - V.view_1d(x, M, origin, span)).max() <= TOL


@pytest.mark.parametrize("N,M,origin,span", [(48, 40, 10.3, 17.9), (45, 64, -3.25, 61.5), (50, 32, 5.5, 77.7), (46, 70, 0.4, 23.0)])
def test_cosine_comes_back_at_the_view_positions(N, M, origin, span):
    """every k the view copies whole (below kmax, and below N/2) comes back as the same cosine at t_m"""
    t = V.positions(M, origin, span)
    kk = V.kmax(N, M, span)
    ks = [k for k in range(0, kk + 1) if 2 * k < N]
    assert 1 in ks
    for k in ks:
        x = 0.5 + 0.3 * np.cos(2 * np.pi * k * np.arange(N) / N + 0.4)
        want = 0.5 + 0.3 * np.cos(2 * np.pi * k * t / N + 0.4)
        assert np.abs(V.view_1d(x, M, origin, span) - want).max() <= TOL, k
    if span > M and kk + 1 < N / 2:
        # s > 1: the first frequency above the output's Nyquist frequency vanishes (no aliasing)
        x = 0.5 + 0.3 * np.cos(2 * np.pi * (kk + 1) * np.arange(N) / N + 0.4)
        assert np.abs(V.view_1d(x, M, origin, span) - 0.5).max() <= TOL


def test_kmax_at_the_ties():
    """span = N: kmax = min(N, M) // 2 for either parity of M -- the exact-size plans' fold (M < N even), split (M > N, N even) and
    kept (M = N) rules follow from it and g"""
    for N in (50, 45, 64, 21):
        for M in (32, 25, 50, 45, 64, 21, 70, 99, 400, 7):
            assert V.kmax(N, M, N) == min(N, M) // 2, (N, M)
    # zooming in never keeps more than the frame has, zooming out keeps what the output can hold
    assert V.kmax(48, 40, 17.9) == 24 and V.kmax(50, 32, 77.7) == int(np.floor(50 * 32 / (2 * 77.7))) == 10
    # one ulp either side of the tie span = N = 2 M (50 -> 25: N M / (2 span) = 12.5) does not matter; at an integer quotient it does
    assert V.kmax(50, 25, np.nextafter(50.0, 0)) == V.kmax(50, 25, 50.0) == V.kmax(50, 25, np.nextafter(50.0, 100)) == 12
    assert V.kmax(48, 24, 48.0) == 12 and V.kmax(48, 24, np.nextafter(48.0, 100)) == 11


def test_shift_by_ffts_is_the_dense_statement():
    x = np.random.default_rng(5).random((2, 21, 32))
    for origin in [(0.5, 0.0), (-3.25, 7.3)]:
        assert np.abs(V.shift_planes(x, origin) - V.view_planes(x, 32, 21, origin, (32.0, 21.0))).max() <= TOL
