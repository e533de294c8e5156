"""CPU checks of the odd-size oracle (tests/oddsize_oracle.py): its FFT form against explicit DFT matrices, against the downscale
oracle where both are defined, and the properties FFTUP_FLAG_ODD_SIZE promises (include/fftup.h).  numpy only, no GPU."""
import numpy as np
import pytest

import downscale_oracle as S
import oddsize_oracle as Q

# (N, M): odd -> even u = 2, even -> odd u = 1.5 (twice), odd -> odd u = 3, odd -> even and even -> odd downscales, u = 1/2 onto
# an odd length, -u 1
PAIRS = [(45, 90), (50, 75), (62, 93), (35, 105), (93, 62), (75, 50), (90, 45), (21, 21)]


@pytest.mark.parametrize("N,M", PAIRS)
def test_fft_form_equals_dft_matrices(N, M):
    x = np.random.RandomState(N + 7 * M).rand(N)
    err = np.abs(Q.resample_matrix(N, M) @ x - Q.resample_1d(x, M)).max()
    print("MEASURED oddsize oracle matrix form %d->%d: max %.3g" % (N, M, err))
    assert err < 1e-12


@pytest.mark.parametrize("N,M", PAIRS)
def test_bin_map_rows_and_columns(N, M):
    """every output bin has at most two sources, every input bin below the shorter Nyquist frequency is used exactly once with
    weight 1, and the map commutes with conjugate symmetry (real in, real out)"""
    B = Q.bin_map(N, M)
    K = min(N, M)
    for k in range(-((K - 1) // 2), (K - 1) // 2 + 1):
        assert B[k % M, k % N] == 1.0 and B[:, k % N].sum() == 1.0
    assert ((B != 0).sum(axis=1) <= 2).all()
    flipM, flipN = (-np.arange(M)) % M, (-np.arange(N)) % N
    assert np.array_equal(B[flipM][:, flipN], B)
    x = np.random.RandomState(N * M).rand(N)
    assert np.abs(np.fft.ifft(Q.map_spectrum(np.fft.fft(x), M)).imag).max() < 1e-14


@pytest.mark.parametrize("N,M", [(92, 46), (64, 32), (60, 40), (100, 80), (16, 2)])
def test_agrees_with_the_downscale_oracle(N, M):
    """even to even, M < N: the downscale flag's rule, unchanged"""
    x = np.random.RandomState(N * 1000 + M).rand(N)
    assert np.abs(Q.resample_1d(x, M) - S.fft_down_1d(x, M)).max() < 1e-13
    assert np.abs(Q.resample_matrix(N, M) - S.fft_down_matrix(N, M)).max() < 1e-13


def test_planes_agree_with_the_downscale_oracle_and_the_per_axis_maps():
    planes = np.random.RandomState(3).rand(3, 24, 40)
    assert np.abs(Q.resample_R(planes, 20, 12) - S.fft_down_R(planes, 20, 12)).max() < 1e-13
    planes = np.random.RandomState(4).rand(3, 21, 45)
    for (uW, uH) in [(90, 42), (67, 31), (45, 21), (30, 14), (22, 63)]:
        AH, AW = Q.resample_matrix(21, uH), Q.resample_matrix(45, uW)
        assert np.abs(Q.resample_R(planes, uW, uH) - np.stack([AH @ p @ AW.T for p in planes])).max() < 1e-12


@pytest.mark.parametrize("N,M", PAIRS)
def test_cosines_below_the_nyquist_bin_come_back_resampled(N, M):
    worst = 0.0
    for k in range((min(N, M) + 1) // 2):                       # every k < min(N, M) / 2
        for a, phi in [(0.3, 0.0), (0.45, 0.7), (0.2, -2.1)]:
            x = 0.5 + a * np.cos(2 * np.pi * k * np.arange(N) / N + phi)
            want = 0.5 + a * np.cos(2 * np.pi * k * np.arange(M) / M + phi)
            worst = max(worst, np.abs(Q.resample_1d(x, M) * M / N - want).max())
    print("MEASURED oddsize oracle cosines %d->%d: max %.3g" % (N, M, worst))
    assert worst < 1e-13


@pytest.mark.parametrize("N,M", PAIRS)
def test_constant_stays_constant(N, M):
    y = Q.resample_planes(np.full((3, 7, N), 0.61), M, 9)
    assert y.shape == (3, 9, M) and np.abs(y - 0.61).max() < 1e-13


@pytest.mark.parametrize("N", [21, 45, 50, 93])
def test_same_length_is_the_identity(N):
    x = np.random.RandomState(N).rand(3, N + 2, N)
    assert np.array_equal(Q.bin_map(N, N), np.eye(N))
    err = np.abs(Q.resample_R(x, N, N + 2) - x).max()
    print("MEASURED oddsize oracle identity %d: max %.3g" % (N, err))
    assert err < 1e-14


def test_output_pixel_m_sits_at_input_position_m_N_over_M():
    """an integer factor keeps the input's samples: every third output pixel of 35 -> 105 is an input pixel"""
    x = np.random.RandomState(9).rand(35)
    assert np.abs(Q.resample_1d(x, 105)[::3] * 3 - x).max() < 1e-13


def test_out_size_is_the_fp32_rule():
    assert [Q.out_size(n, u) for n, u in [(45, 2.0), (50, 1.5), (75, 1.4), (45, 1.4), (125, 0.6), (75, 0.6), (62, 1.5), (38, 1.5)]] == \
        [90, 75, 105, 63, 75, 45, 93, 57]
