"""fp64 oracle of the odd-size mode (FFTUP_FLAG_ODD_SIZE, include/fftup.h).  numpy only: no scipy, no GPU.

Exact trigonometric resampling per axis, separable (scipy.signal.resample's rule).  Input x[n] (n < N), output length M (either
parity, above, below or equal to N), X = DFT_N(x) unnormalised, K = min(N, M):
    bins |k| < K/2 are copied:             Y[k mod M] = X[k mod N];
    K even, its Nyquist bin h = K/2:       M > N: split, Y[h] = Y[M-h] = X[h]/2;   M < N: folded, Y[h] = X[h] + X[N-h];   M = N: kept;
    every other bin of Y is 0,
and R = (1/M) IDFT_M(Y) per axis -- what the kernels store as the pre-sharpen image.  The amplitude-preserving image is
y = R (uW uH) / (W H): output pixel m sits at input position m N / M.
"""
import numpy as np


def out_size(n, u):
    """(uint32_t)(u n) in fp32, as fftup_plan_create computes it"""
    return int(np.float32(u) * np.float32(n))


def bin_map(N, M):
    """S [M][N] with Y = S X: the rule above as a matrix of 0, 1/2 and 1"""
    S = np.zeros((M, N))
    K = min(N, M)
    for k in range(-((K - 1) // 2), (K - 1) // 2 + 1):                  # |k| < K/2
        S[k % M, k % N] = 1.0
    if K % 2 == 0:
        h = K // 2
        if M > N:
            S[h, h] = S[M - h, h] = 0.5
        elif M < N:
            S[h, h] = S[h, N - h] = 1.0
        else:
            S[h, h] = 1.0
    return S


def map_spectrum(X, M, axis=-1):
    """Y of length M from the length-N spectrum X along `axis`, by slices (no matrix)"""
    X = np.moveaxis(np.asarray(X, dtype=np.complex128), axis, -1)
    N = X.shape[-1]
    K = min(N, M)
    p = (K - 1) // 2                                                    # copied bins: -p .. p
    Y = np.zeros(X.shape[:-1] + (M,), np.complex128)
    Y[..., :p + 1] = X[..., :p + 1]
    if p:
        Y[..., M - p:] = X[..., N - p:]
    if K % 2 == 0:
        h = K // 2
        if M > N:
            Y[..., h] = Y[..., M - h] = 0.5 * X[..., h]
        elif M < N:
            Y[..., h] = X[..., h] + X[..., N - h]
        else:
            Y[..., h] = X[..., h]
    return np.moveaxis(Y, -1, axis)


def resample_1d(x, M):
    """R of one axis: (1/M) IDFT_M of the mapped spectrum (real input: real output)"""
    return np.real(np.fft.ifft(map_spectrum(np.fft.fft(np.asarray(x, dtype=np.float64)), M)))


def dft_matrix(N, sign=-1):
    n = np.arange(N)
    return np.exp(sign * 2j * np.pi * np.outer(n, n) / N)


def resample_matrix(N, M):
    """the same map as a matrix [M][N], from explicit DFT matrices: (1/M) IDFT_M . bin_map . DFT_N"""
    return np.real(dft_matrix(M, +1) @ bin_map(N, M) @ dft_matrix(N, -1)) / M


def resample_R(planes, uW, uH):
    """planes [C][H][W] -> R [C][uH][uW] (fp64): both axes through the complex transform, one plane at a time"""
    planes = np.asarray(planes, dtype=np.float64)
    out = []
    for p in planes:
        Y = map_spectrum(map_spectrum(np.fft.fft2(p), uW, axis=1), uH, axis=0)
        out.append(np.real(np.fft.ifft2(Y)))
    return np.stack(out)


def resample_planes(planes, uW, uH):
    """the amplitude-preserving image y = R (uW uH) / (W H)"""
    _, H, W = np.shape(planes)
    return resample_R(planes, uW, uH) * (uW * uH) / (W * H)
