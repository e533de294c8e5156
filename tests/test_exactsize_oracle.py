"""CPU: the fp64 oracle of the exact-size plans, tests/exactsize_oracle.py -- exact trigonometric resampling per axis with an
optional alignment of the pixel centres.  Every property below is one the kernels inherit from the rule; fp64 rounding of
transforms of up to 1920 points stays below 1e-12."""
import numpy as np
import pytest

import exactsize_oracle as E
import oddsize_oracle as Q

PAIRS = [(46, 70), (40, 25), (50, 32), (32, 50), (45, 64), (21, 21), (48, 30), (1366, 1920)]
TOL = 1e-12


def _row(N, seed=0):
    return np.random.RandomState(seed + N).rand(N)


@pytest.mark.parametrize("N,M", PAIRS)
def test_corner_alignment_is_the_oddsize_rule(N, M):
    x = _row(N)
    assert np.abs(E.resample_1d(x, M, E.ALIGN_CORNER).real - Q.resample_1d(x, M)).max() <= TOL
    planes = np.random.RandomState(N * M).rand(2, 12, N)
    assert np.abs(E.resample_R(planes, M, 9, E.ALIGN_CORNER) - Q.resample_R(planes, M, 9)).max() <= TOL
    assert np.abs(E.resample_planes(planes, M, 9, E.ALIGN_CORNER) - Q.resample_planes(planes, M, 9)).max() <= TOL


@pytest.mark.parametrize("align", [E.ALIGN_CORNER, E.ALIGN_CENTRE])
@pytest.mark.parametrize("N,M", PAIRS)
def test_slices_equal_the_explicit_dft_matrices(N, M, align):
    x = _row(N, 1)
    A = E.resample_matrix(N, M, align)
    assert np.abs(A.imag).max() <= TOL                      # a real map
    assert np.abs(A @ x - E.resample_1d(x, M, align)).max() <= TOL


@pytest.mark.parametrize("align", [E.ALIGN_CORNER, E.ALIGN_CENTRE])
@pytest.mark.parametrize("N,M", PAIRS)
def test_real_input_gives_real_output(N, M, align):
    y = E.resample_1d(_row(N, 2), M, align)
    assert np.abs(y.imag).max() <= TOL


@pytest.mark.parametrize("N,M", PAIRS)
def test_centre_alignment_commutes_with_mirroring(N, M):
    x = _row(N, 3)
    a = E.resample_1d(x[::-1], M, E.ALIGN_CENTRE).real
    b = E.resample_1d(x, M, E.ALIGN_CENTRE).real[::-1]
    assert np.abs(a - b).max() <= TOL
    # ... in two dimensions, both axes mirrored
    p = np.random.RandomState(N + M).rand(1, 10, N)
    a = E.resample_R(p[:, ::-1, ::-1], M, 15, E.ALIGN_CENTRE)
    b = E.resample_R(p, M, 15, E.ALIGN_CENTRE)[:, ::-1, ::-1]
    assert np.abs(a - b).max() <= TOL


@pytest.mark.parametrize("N,M", [p for p in PAIRS if p[0] != p[1]])
def test_corner_alignment_does_not(N, M):
    """why the centre rule exists: under the corner rule the same comparison is off by a good part of full scale"""
    x = _row(N, 3)
    a = E.resample_1d(x[::-1], M, E.ALIGN_CORNER).real
    b = E.resample_1d(x, M, E.ALIGN_CORNER).real[::-1]
    assert np.abs(a - b).max() >= 0.1


@pytest.mark.parametrize("align", [E.ALIGN_CORNER, E.ALIGN_CENTRE])
@pytest.mark.parametrize("N,M", PAIRS)
def test_a_cosine_comes_back_at_the_output_positions(N, M, align):
    """k cycles, k below min(N, M)/2 (a bin that is copied): the same cosine, sampled at (m + 1/2) N / M - 1/2 (centres) or m N / M"""
    K = min(N, M)
    pos = E.positions(N, M, align)
    if align == E.ALIGN_CENTRE:
        assert np.allclose(pos, (np.arange(M) + 0.5) * N / M - 0.5, rtol=0, atol=1e-12)
    for k in sorted({0, 1, (K - 1) // 2}):
        for theta in (0.0, 0.7):
            x = 0.5 + 0.3 * np.cos(2 * np.pi * k * np.arange(N) / N + theta)
            want = 0.5 + 0.3 * np.cos(2 * np.pi * k * pos / N + theta)
            assert np.abs(E.resample_1d(x, M, align).real * M / N - want).max() <= TOL, (k, theta)      # (y = R M / N)


@pytest.mark.parametrize("align", [E.ALIGN_CORNER, E.ALIGN_CENTRE])
@pytest.mark.parametrize("N,M", PAIRS)
def test_constants_and_identity(N, M, align):
    assert np.abs(E.resample_1d(np.full(N, 0.37), M, align) * M / N - 0.37).max() <= TOL
    x = _row(N, 4)
    assert np.abs(E.resample_1d(x, N, align) - x).max() <= TOL            # M = N: d = 0, the identity at both alignments
    p = np.random.RandomState(7).rand(3, 6, N)
    assert np.abs(E.resample_R(p, N, 6, align) - p).max() <= TOL
    assert np.abs(E.resample_planes(np.full((1, 8, N), 0.25), M, 13, align) - 0.25).max() <= TOL


def test_effective_factor():
    assert E.effective_factor(1215, 675, 2430, 1350) == 2.0
    assert E.effective_factor(36, 20, 36, 20) == 1.0
    u = E.effective_factor(1366, 768, 1920, 1080)
    assert u == float(np.float32(np.sqrt(1920 * 1080 / (1366 * 768)))) and abs(u - 1.4059) < 1e-4
