"""fp64 oracle of the downscale mode (FFTUP_FLAG_DOWNSCALE, include/fftup.h).  numpy only: no scipy, no GPU.

FFT mode, per axis, separable: input x[n] (n < N), output length M < N (both even), h = M/2, X = DFT(x) unnormalised.  The
spectrum is cropped with its Nyquist bins folded,
    Y[k] = X[k] (k < h),   Y[h] = X[h] + X[N-h],   Y[M-k] = X[N-k] (0 < k < h),
and R = (1/M) IDFT_M(Y) per axis -- what the kernels store as the pre-sharpen image.  The amplitude-preserving image is
y = R (uW uH) / (W H).

DCT mode (FFTUP_FLAG_DCT | FFTUP_FLAG_DOWNSCALE): the DCT mode's formula with the coefficients truncated,
    y[m] = X[0]/N + (2/N) sum_{k=1}^{M-1} X[k] cos(pi k (2m+1) / 2M),   X = DCT-II(x),   R = y / upsq.
(dct_oracle.resample_matrix sums k < N: for M < N that aliases, hence the truncated matrix here.)
"""
import numpy as np

import dct_oracle as D

out_size = D.out_size
upsq = D.upsq


# ---- FFT mode
def crop_spectrum(X, M, axis=-1):
    """Y of length M from the length-N spectrum X along `axis`: bins below h, the folded Nyquist bin, the top h - 1 bins"""
    X = np.moveaxis(np.asarray(X, dtype=np.complex128), axis, -1)
    N, h = X.shape[-1], M // 2
    Y = np.zeros(X.shape[:-1] + (M,), np.complex128)
    Y[..., :h] = X[..., :h]
    Y[..., h] = X[..., h] + X[..., N - h]
    if h > 1:
        Y[..., M - h + 1:] = X[..., N - h + 1:]
    return np.moveaxis(Y, -1, axis)


def fft_down_1d(x, M):
    """R of one axis, (1/M) IDFT_M of the cropped spectrum (real input: real output)"""
    return np.real(np.fft.ifft(crop_spectrum(np.fft.fft(np.asarray(x, dtype=np.float64)), M)))


def dft_matrix(N, sign=-1):
    n = np.arange(N)
    return np.exp(sign * 2j * np.pi * np.outer(n, n) / N)


def fft_down_matrix(N, M):
    """the same map as a matrix [M][N], from explicit DFT matrices: (1/M) IDFT_M . crop . DFT_N"""
    S = np.zeros((M, N))
    h = M // 2
    for k in range(h):
        S[k, k] = 1.0
    S[h, h] += 1.0
    S[h, N - h] += 1.0
    for k in range(1, h):
        S[M - k, N - k] = 1.0
    return np.real(dft_matrix(M, +1) @ S @ dft_matrix(N, -1)) / M


def fft_down_R(planes, uW, uH):
    """planes [C][H][W] -> R [C][uH][uW] (fp64): rows through rfft (the kernels' half spectrum, Nyquist bin 2 Re X[h]), columns
    through the complex transform, one plane at a time"""
    planes = np.asarray(planes, dtype=np.float64)
    h = uW // 2
    out = []
    for p in planes:
        X = np.fft.rfft(p, axis=-1)[:, :h + 1]
        X[:, h] = 2.0 * X[:, h].real                                      # X[h] + X[W-h] of a real row
        Z = np.fft.ifft(crop_spectrum(np.fft.fft(X, axis=0), uH, axis=0), axis=0)
        out.append(np.fft.irfft(Z, n=uW, axis=-1))
    return np.stack(out)


def fft_down_planes(planes, uW, uH):
    """the amplitude-preserving image y = R (uW uH) / (W H)"""
    _, H, W = np.shape(planes)
    return fft_down_R(planes, uW, uH) * (uW * uH) / (W * H)


# ---- DCT mode
def dct3_trunc_matrix(N, M):
    k, m = np.arange(M), np.arange(M)
    c = np.full(M, 2.0 / N)
    c[0] = 1.0 / N
    return np.cos(np.pi * np.outer(2 * m + 1, k) / (2 * M)) * c                   # [m][k], k < M


def dct_down_matrix(N, M):
    """y = A x: DCT-II of length N, the first M coefficients, DCT-III of length M"""
    return dct3_trunc_matrix(N, M) @ D.dct2_matrix(N)[:M]


def dct_down_planes(planes, uW, uH):
    """planes [C][H][W] -> y [C][uH][uW] (fp64), the DCT downscale image before sharpening (upsq * R)"""
    planes = np.asarray(planes, dtype=np.float64)
    _, H, W = planes.shape
    AH, AW = dct_down_matrix(H, uH), dct_down_matrix(W, uW)
    return np.stack([AH @ p @ AW.T for p in planes])
