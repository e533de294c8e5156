"""fp64 oracle of the exact-size plans (fftup_plan_create_size, include/fftup.h).  numpy only: no scipy, no GPU.

Exact trigonometric resampling per axis, separable -- the rule of oddsize_oracle -- with an optional alignment of the pixel
CENTRES.  Per axis, input x[n] (n < N), output length M (either parity, above, below or equal to N), X = DFT_N(x) unnormalised,
K = min(N, M), d = (N/M - 1)/2 for ALIGN_CENTRE and 0 for ALIGN_CORNER.  The bin of signed frequency f carries exp(2 pi i f d / N):
    bins |f| < K/2 are copied:             Y[f mod M] = X[f mod N] exp(2 pi i f d / N);
    K even, its Nyquist bin h = K/2, phi = 2 pi h d / N:
        M > N: split,   Y[h] = X[h] exp(+i phi) / 2,  Y[M-h] = X[h] exp(-i phi) / 2;
        M < N: folded,  Y[h] = X[h] exp(+i phi) + X[N-h] exp(-i phi);
        M = N: kept (d = 0);
    every other bin of Y is 0,
and R = (1/M) IDFT_M(Y) per axis -- what the kernels store as the pre-sharpen image.  The amplitude-preserving image is
y = R (uW uH) / (W H): output pixel m sits at input position (m + 1/2) N / M - 1/2 (centres) or m N / M (corners).
"""
import numpy as np

import oddsize_oracle as OD

ALIGN_CORNER = 0
ALIGN_CENTRE = 1


def delta(N, M, align):
    """shift of the sampling grid in input pixels"""
    return (N / M - 1.0) / 2.0 if align == ALIGN_CENTRE else 0.0


def positions(N, M, align):
    """input positions of the M output pixels"""
    return np.arange(M) * (N / M) + delta(N, M, align)


def effective_factor(W, H, uW, uH):
    """u_e = (float)sqrt((double)uW uH / ((double)W H)): what the sharpen constant is computed from"""
    return float(np.float32(np.sqrt(float(uW) * float(uH) / (float(W) * float(H)))))


def map_spectrum(X, M, align=ALIGN_CORNER, axis=-1):
    """Y of length M from the length-N spectrum X along `axis`, by slices"""
    X = np.moveaxis(np.asarray(X, dtype=np.complex128), axis, -1)
    N = X.shape[-1]
    K = min(N, M)
    d = delta(N, M, align)
    p = (K - 1) // 2                                                    # copied bins: -p .. p
    ph = np.exp(2j * np.pi * np.arange(K // 2 + 1) * d / N)             # factor of the frequency +f; -f takes the conjugate
    Y = np.zeros(X.shape[:-1] + (M,), np.complex128)
    Y[..., :p + 1] = X[..., :p + 1] * ph[:p + 1]
    if p:
        Y[..., M - p:] = X[..., N - p:] * np.conj(ph[p:0:-1])
    if K % 2 == 0:
        h = K // 2
        if M > N:
            Y[..., h] = 0.5 * X[..., h] * ph[h]
            Y[..., M - h] = 0.5 * X[..., h] * np.conj(ph[h])
        elif M < N:
            Y[..., h] = X[..., h] * ph[h] + X[..., N - h] * np.conj(ph[h])
        else:
            Y[..., h] = X[..., h]
    return np.moveaxis(Y, -1, axis)


def resample_1d(x, M, align=ALIGN_CORNER):
    """R of one axis, complex (the imaginary part of a real input's result is rounding noise: the tests check that)"""
    return np.fft.ifft(map_spectrum(np.fft.fft(np.asarray(x, dtype=np.float64)), M, align))


def resample_matrix(N, M, align=ALIGN_CORNER):
    """the same map as a matrix [M][N] from explicit DFT matrices, bin by bin (complex; real up to rounding)"""
    d = delta(N, M, align)
    K = min(N, M)
    S = np.zeros((M, N), np.complex128)
    for f in range(-((K - 1) // 2), (K - 1) // 2 + 1):
        S[f % M, f % N] = np.exp(2j * np.pi * f * d / N)
    if K % 2 == 0:
        h = K // 2
        e = np.exp(2j * np.pi * h * d / N)
        if M > N:
            S[h, h] = 0.5 * e
            S[M - h, h] = 0.5 * np.conj(e)
        elif M < N:
            S[h, h] = e
            S[h, N - h] = np.conj(e)
        else:
            S[h, h] = 1.0
    return OD.dft_matrix(M, +1) @ S @ OD.dft_matrix(N, -1) / M


def resample_R(planes, uW, uH, align=ALIGN_CORNER):
    """planes [C][H][W] -> R [C][uH][uW] (fp64)"""
    planes = np.asarray(planes, dtype=np.float64)
    out = []
    for p in planes:
        Y = map_spectrum(map_spectrum(np.fft.fft2(p), uW, align, axis=1), uH, align, axis=0)
        out.append(np.real(np.fft.ifft2(Y)))
    return np.stack(out)


def resample_planes(planes, uW, uH, align=ALIGN_CORNER):
    """the amplitude-preserving image y = R (uW uH) / (W H)"""
    _, H, W = np.shape(planes)
    return resample_R(planes, uW, uH, align) * (uW * uH) / (W * H)
