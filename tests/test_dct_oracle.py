"""CPU checks of the DCT-mode oracle (tests/dct_oracle.py): its matrix form against the FFT (Makhoul) form the kernels compute,
and the properties FFTUP_FLAG_DCT promises (include/fftup.h).  No GPU, no scipy."""
import numpy as np
import pytest

import dct_oracle as D

# (N, M): u = 2, u = 1.5, u = 1, 3*5*7-smooth lengths, u < 2 where the two bands of the DCT-III input overlap
SIZES = [(8, 16), (64, 128), (60, 90), (105, 210), (210, 630), (42, 56), (16, 16), (10, 14), (240, 300)]


@pytest.mark.parametrize("N,M", SIZES)
def test_matrix_form_equals_fft_form(N, M):
    x = np.random.RandomState(N * 1000 + M).rand(N)
    assert np.abs(D.dct2_matrix(N) @ x - D.dct2_fft(x)).max() <= 1e-12 * N
    assert np.abs(D.resample_1d(x, M) - D.resample_1d_fft(x, M)).max() <= 1e-12


@pytest.mark.parametrize("N", [8, 30, 64, 105])
def test_unit_factor_is_identity(N):
    x = np.random.RandomState(N).rand(N)
    assert np.abs(D.resample_1d(x, N) - x).max() <= 1e-12


@pytest.mark.parametrize("N,M", SIZES)
def test_constant_stays_constant(N, M):
    assert np.abs(D.resample_1d(np.full(N, 0.37), M) - 0.37).max() <= 1e-12
    y = D.resample_planes(np.full((3, 6, N), 0.61), M, 10)
    assert y.shape == (3, 10, M) and np.abs(y - 0.61).max() <= 1e-12


@pytest.mark.parametrize("N,M", SIZES)
def test_dct_cosine_resamples_exactly(N, M):
    for k in (0, 1, N // 3, N - 1):
        x = np.cos(np.pi * k * (2 * np.arange(N) + 1) / (2 * N))
        y = np.cos(np.pi * k * (2 * np.arange(M) + 1) / (2 * M))
        assert np.abs(D.resample_1d(x, M) - y).max() <= 1e-11


@pytest.mark.parametrize("N", [64, 96, 128])
def test_ramp_has_no_border_ringing(N):
    """a linear ramp 0..1: the DCT interpolant follows the ramp (at the pixel-centre positions) to 3e-3 everywhere, the
    FFT path's periodic interpolant wraps the 1 -> 0 step at the seam and overshoots by more than 0.1 at both ends"""
    M = 2 * N
    x = np.arange(N) / (N - 1.0)
    y = D.resample_1d(x, M)
    err = np.abs(y - D.centre_positions(N, M) / (N - 1.0)).max()
    f = D.fft_resample_1d(x, M)
    overshoot = max(f.max() - 1.0, -f.min())
    print("MEASURED dct_ramp N=%d: dct_max_err %.3g  fft_overshoot %.3g" % (N, err, overshoot))
    assert err <= 3e-3
    assert overshoot > 0.1


def test_sizes_and_upsq_helpers():
    assert D.out_size(1920, 2.0) == 3840 and D.out_size(96, 1.5) == 144 and D.out_size(210, 1.25) == 262
    assert D.upsq(2.0) == 4.0 and D.upsq(1.5) == 2.25 and D.upsq(3.0) == 9.0
    # "%f" keeps six decimals: 1.1^2 = 1.2100000381... in fp32 -> "1.210000"
    assert D.upsq(1.1) == float(np.float32(1.21))
    assert D.upsq(1.1, half=True) == float(np.float16(np.float32(1.21)))
