"""fp64 oracle of the DCT upscale mode (FFTUP_FLAG_DCT, include/fftup.h).  numpy only: no scipy, no GPU.

Per axis, separable, input x[n] (n < N), output y[m] (m < M):
    X[k] = sum_n x[n] cos(pi k (2n+1) / 2N)                                       (DCT-II, unnormalised)
    y[m] = X[0]/N + (2/N) sum_{k=1}^{N-1} X[k] cos(pi k (2m+1) / 2M)              (DCT-III of the zero-padded coefficients)
The matrix form of that definition is the oracle; the FFT (Makhoul) form is what the kernels compute, kept here so that the
CPU tests can show the two agree.
"""
import numpy as np


def dct2_matrix(N):
    n = np.arange(N)
    return np.cos(np.pi * np.outer(n, 2 * n + 1) / (2 * N))                        # [k][n]


def dct3_pad_matrix(N, M):
    k, m = np.arange(N), np.arange(M)
    c = np.full(N, 2.0 / N)
    c[0] = 1.0 / N
    return np.cos(np.pi * np.outer(2 * m + 1, k) / (2 * M)) * c                     # [m][k]


def resample_matrix(N, M):
    """y = A x: DCT-II of length N, zero-pad, DCT-III of length M"""
    return dct3_pad_matrix(N, M) @ dct2_matrix(N)


def resample_1d(x, M):
    x = np.asarray(x, dtype=np.float64)
    return resample_matrix(x.shape[-1], M) @ x


def resample_planes(planes, uW, uH):
    """planes [C][H][W] -> y [C][uH][uW] (fp64), the DCT-mode image before sharpening (upsq * R)"""
    planes = np.asarray(planes, dtype=np.float64)
    _, H, W = planes.shape
    AH, AW = resample_matrix(H, uH), resample_matrix(W, uW)
    return np.stack([AH @ p @ AW.T for p in planes])


# ---- the FFT form (Makhoul): what k_dct_row / k_dct_col / k_idct_row compute
def dct2_fft(x):
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[-1]
    v = np.empty(N)
    v[:(N + 1) // 2] = x[0::2]
    v[N - 1 - np.arange(N // 2)] = x[1::2]
    k = np.arange(N)
    return np.real(np.exp(-1j * np.pi * k / (2 * N)) * np.fft.fft(v))


def dct3_pad_fft(X, M):
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[-1]
    C = np.zeros(M)
    C[:N] = X * (2.0 / N)
    C[0] = X[0] / N
    k = np.arange(M)
    Crev = np.zeros(M)
    Crev[1:] = C[M - k[1:]]
    Wk = 0.5 * np.exp(1j * np.pi * k / (2 * M)) * (C - 1j * Crev)
    Wk[0] = C[0]
    w = np.fft.ifft(Wk) * M                                                       # sum_k W[k] e^{+2 pi i k n / M}
    assert np.abs(w.imag).max() <= 1e-9 * max(1.0, np.abs(w.real).max())
    y = np.empty(M)
    y[0::2] = w.real[:(M + 1) // 2]
    y[1::2] = w.real[M - 1 - np.arange(M // 2)]
    return y


def resample_1d_fft(x, M):
    return dct3_pad_fft(dct2_fft(x), M)


def fft_resample_1d(x, M):
    """the FFT path's interpolant (periodic, pixel 0 on pixel 0), for comparison: centred zero-padding, Nyquist bin split"""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[-1]
    X = np.fft.fft(x)
    Y = np.zeros(M, dtype=complex)
    h = N // 2
    Y[:h] = X[:h]
    Y[M - h + 1:] = X[h + 1:]
    Y[h] += 0.5 * X[h]
    Y[M - h] += 0.5 * X[h]
    return np.real(np.fft.ifft(Y)) * (M / N)


def out_size(n, u):
    """the output-size rule of both paths: (uint32_t)(u * n) in fp32"""
    return int(np.float32(u) * np.float32(n))


def centre_positions(N, M):
    """input position of output pixel m in the DCT mode: (m + 1/2) N / M - 1/2"""
    return (np.arange(M) + 0.5) * N / M - 0.5


def upsq(u, half=False):
    """the plan's sharpen constant P->upsq: the fp32 product u*u through "%f" text (const_via_percent_f), binary16 for -p 2"""
    v = np.float32(u) * np.float32(u)
    f = np.float32(float("%f" % float(v)))
    if half:
        f = np.float32(np.float16(f))
    return float(f)
