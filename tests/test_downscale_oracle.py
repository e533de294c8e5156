"""CPU checks of the downscale oracle (tests/downscale_oracle.py): its FFT form against scipy.signal.resample and against explicit
DFT matrices, and the properties FFTUP_FLAG_DOWNSCALE promises (include/fftup.h).  No GPU."""
import numpy as np
import pytest

import dct_oracle as D
import downscale_oracle as S

# (N, M): u = 1/2, 1/4, 3/4, 2/3, 1/8, 0.8, smallest output, 3*5*7-smooth lengths
SIZES = [(8, 4), (64, 32), (64, 16), (60, 40), (96, 64), (128, 16), (100, 80), (16, 2), (840, 420), (210, 70)]


@pytest.mark.parametrize("N,M", SIZES)
def test_fft_form_equals_scipy_resample(N, M):
    signal = pytest.importorskip("scipy.signal")
    x = np.random.RandomState(N * 1000 + M).rand(N)
    y = S.fft_down_1d(x, M) * M / N
    assert np.abs(y - signal.resample(x, M)).max() <= 1e-12


@pytest.mark.parametrize("N,M", SIZES)
def test_fft_form_equals_dft_matrices(N, M):
    x = np.random.RandomState(N + 7 * M).rand(N)
    assert np.abs(S.fft_down_matrix(N, M) @ x - S.fft_down_1d(x, M)).max() <= 1e-12


def test_planes_equal_per_axis_maps():
    """the rfft / complex-column form of fft_down_R is the separable per-axis map, and it agrees with scipy on both axes"""
    rng = np.random.RandomState(3)
    planes = rng.rand(3, 24, 40)
    R = S.fft_down_R(planes, 20, 12)
    AH, AW = S.fft_down_matrix(24, 12), S.fft_down_matrix(40, 20)
    assert np.abs(R - np.stack([AH @ p @ AW.T for p in planes])).max() <= 1e-12
    signal = pytest.importorskip("scipy.signal")
    want = signal.resample(signal.resample(planes, 20, axis=2), 12, axis=1)
    assert np.abs(S.fft_down_planes(planes, 20, 12) - want).max() <= 1e-12


@pytest.mark.parametrize("N,M", SIZES)
def test_constant_stays_constant(N, M):
    y = S.fft_down_planes(np.full((3, 6, N), 0.61), M, 4)
    assert y.shape == (3, 4, M) and np.abs(y - 0.61).max() <= 1e-12
    y = S.dct_down_planes(np.full((3, 6, N), 0.61), M, 4)
    assert np.abs(y - 0.61).max() <= 1e-12


@pytest.mark.parametrize("d", [2, 4])
def test_band_limited_frame_decimates_exactly(d):
    """no energy at or above the new Nyquist frequency: the output is every d-th pixel (pixel 0 on pixel 0)"""
    H, W = 32, 48
    rng = np.random.RandomState(d)
    x = np.zeros((3, H, W))
    for _ in range(12):
        ky, kx = rng.randint(-(H // d) // 2 + 1, (H // d) // 2), rng.randint(-(W // d) // 2 + 1, (W // d) // 2)
        yy, xx = np.mgrid[0:H, 0:W]
        x += rng.rand() * np.cos(2 * np.pi * (ky * yy / H + kx * xx / W) + rng.rand() * 6.28)
    y = S.fft_down_planes(x, W // d, H // d)
    assert np.abs(y - x[:, ::d, ::d]).max() <= 1e-12


def test_content_above_new_nyquist_vanishes():
    """a cosine at 0.375 cycles per pixel (above the 0.25 of u = 1/2) leaves nothing but the mean"""
    N = 64
    n = np.arange(N)
    x = 0.5 + 0.3 * np.cos(2 * np.pi * 0.375 * n + 0.4)
    planes = np.broadcast_to(x, (3, 8, N)) * np.broadcast_to(x[:8, None], (3, 8, N))
    y = S.fft_down_planes(planes, N // 2, 4)
    assert np.abs(y - 0.25).max() <= 1e-12
    assert np.abs(S.fft_down_1d(x, 32) * 0.5 - 0.5).max() <= 1e-12


@pytest.mark.parametrize("N,M", [(8, 16), (60, 90), (64, 128), (105, 210), (42, 56), (16, 128)])
def test_dct_down_after_up_is_identity(N, M):
    x = np.random.RandomState(N + M).rand(N)
    assert np.abs(S.dct_down_matrix(M, N) @ D.resample_matrix(N, M) @ x - x).max() <= 1e-12


@pytest.mark.parametrize("N,M", SIZES)
def test_dct_down_is_the_truncated_dct(N, M):
    """the DCT-III of the first M DCT-II coefficients, written out; a DCT cosine of index k < M resamples exactly"""
    x = np.random.RandomState(5 * N + M).rand(N)
    X = D.dct2_matrix(N) @ x
    m = np.arange(M)
    y = X[0] / N + (2.0 / N) * sum(X[k] * np.cos(np.pi * k * (2 * m + 1) / (2 * M)) for k in range(1, M))
    assert np.abs(S.dct_down_matrix(N, M) @ x - y).max() <= 1e-12
    for k in (0, 1, M // 2, M - 1):
        xc = np.cos(np.pi * k * (2 * np.arange(N) + 1) / (2 * N))
        assert np.abs(S.dct_down_matrix(N, M) @ xc - np.cos(np.pi * k * (2 * m + 1) / (2 * M))).max() <= 1e-11


def test_sizes_of_the_issue_are_even_and_smooth():
    def smooth(n):
        for p in (2, 3, 5, 7):
            while n % p == 0:
                n //= p
        return n == 1
    for W, H, u in ((4096, 2048, 0.5), (2560, 1440, 0.75), (1920, 1080, 2 / 3), (840, 336, 0.5), (2048, 1024, 0.125),
                    (1000, 800, 0.8), (7680, 4320, 0.5)):
        uW, uH = S.out_size(W, u), S.out_size(H, u)
        assert uW % 2 == 0 and uH % 2 == 0 and smooth(uW) and smooth(uH) and uW < W and uH < H, (W, H, u)
    assert (S.out_size(1920, 2 / 3), S.out_size(1080, 2 / 3)) == (1280, 720)
    assert S.upsq(0.5) == 0.25 and S.upsq(0.125) == 0.015625 and S.upsq(0.75) == 0.5625
