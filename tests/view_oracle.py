"""fp64 oracle of the view plans (fftup_plan_create_view, include/fftup.h).  numpy only: no scipy, no GPU.

Per axis, separable: input x[n] (n < N), X[f] = sum_n x[n] exp(-2 pi i nf / N), an output of M points and a view (origin, span) in
doubles, step s = span / M.  Output pixel m sits at input position t_m = origin + m s (pixel indices as coordinates, the frame
periodic with period N), and
    kmax = min(N // 2, floor((double)(N M) / (2 max(span, (double)M))))
    g_f  = 1/2 if 2 |f| == N else 1
    y[m] = (1/N) sum_{f = -kmax .. kmax} g_f X[f mod N] exp(2 pi i f t_m / N)
-- the frame's trigonometric interpolant at t_m for s <= 1, truncated at the output's Nyquist frequency for s > 1.  Stated as a
dense matrix [M][N], evaluated directly (no chirp, no FFT).  The pre-sharpen image the kernels store is
R = y span_x span_y / (uW uH); the sharpen pass takes the effective factor u_e = (float)sqrt((double)uW uH / (span_x span_y)).
"""
import numpy as np


def kmax(N, M, span):
    """the last bin kept, in double exactly as the header writes it (N M is exact, the quotient correctly rounded)"""
    return int(min(N // 2, np.floor(float(N * M) / (2.0 * max(float(span), float(M))))))


def smooth_from(n):
    """the smallest 2,3,5,7-smooth length >= n"""
    def smooth(q):
        for p in (2, 3, 5, 7):
            while q % p == 0:
                q //= p
        return q == 1
    while not smooth(n):
        n += 1
    return n


def conv_length(N, M):
    """the convolution length of an axis: the smallest 2,3,5,7-smooth L >= 2 (N // 2) + M (the worst case kmax = N // 2)"""
    return smooth_from(2 * (N // 2) + M)


def positions(M, origin, span):
    """input positions of the M output pixels"""
    return float(origin) + np.arange(M) * (float(span) / M)


def view_factors(N, M, origin, span):
    """the two factors of the dense statement, V = E F / N: E [M][K] evaluates the kept bins at the positions, F [K][N] is the
    DFT's rows of those bins (for lengths of thousands, where E (F x) / N costs a thousandth of forming V)"""
    k = kmax(N, M, span)
    f = np.arange(-k, k + 1)
    g = np.where(2 * np.abs(f) == N, 0.5, 1.0)
    t = positions(M, origin, span)
    E = np.exp(2j * np.pi * np.outer(t, f) / N) * g                    # [M][K]
    F = np.exp(-2j * np.pi * np.outer(f, np.arange(N)) / N)            # [K][N]: X[f mod N] = sum_n x[n] exp(-2 pi i nf / N)
    return E, F


def view_matrix(N, M, origin, span):
    """y = V x, V [M][N] complex (real up to rounding: the tests check that)"""
    E, F = view_factors(N, M, origin, span)
    return E @ F / N


def view_1d(x, M, origin, span):
    return view_matrix(len(x), M, origin, span) @ np.asarray(x, dtype=np.float64)


def view_planes(planes, uW, uH, origin, span):
    """planes [C][H][W] -> the amplitude-preserving image y [C][uH][uW] (fp64); origin = (x, y), span = (x, y)"""
    planes = np.asarray(planes, dtype=np.float64)
    _, H, W = planes.shape
    Vx = np.real(view_matrix(W, uW, origin[0], span[0]))
    Vy = np.real(view_matrix(H, uH, origin[1], span[1]))
    return Vy @ planes @ Vx.T


def shift_planes(planes, origin):
    """view_planes for uW = W, uH = H, span = (W, H) -- a shift of the lattice by `origin` -- through FFTs instead of dense matrices
    (for lengths of thousands): the bin of frequency f takes exp(2 pi i f origin / N), an even N's Nyquist bin cos(pi origin)"""
    out = np.fft.fft2(np.asarray(planes, dtype=np.float64))
    for axis, o in ((2, origin[0]), (1, origin[1])):
        N = out.shape[axis]
        f = np.fft.fftfreq(N, 1.0 / N)
        ph = np.exp(2j * np.pi * f * float(o) / N)
        if N % 2 == 0:
            ph[N // 2] = np.cos(np.pi * float(o))
        out = out * ph.reshape([-1 if a == axis else 1 for a in range(3)])
    return np.real(np.fft.ifft2(out))


def view_R(planes, uW, uH, origin, span):
    """the pre-sharpen image R = y span_x span_y / (uW uH)"""
    return view_planes(planes, uW, uH, origin, span) * (float(span[0]) * float(span[1]) / (uW * uH))


def effective_factor(uW, uH, span):
    """u_e = (float)sqrt((double)uW uH / (span_x span_y)): what the sharpen constant is computed from"""
    return float(np.float32(np.sqrt(float(uW) * float(uH) / (float(span[0]) * float(span[1])))))


def chirp_tables(N, M, origin, span):
    """the chirp-z factorisation of the same map (csrc/kernels_view.hpp) in longdouble: (kmax, pre [K], post [M], c [K + M - 1] for
    d = -(K - 1) .. M - 1), with y[m] = post[m] sum_j Z_j pre[j] c[m - j], Z_j = X[(j - kmax) mod N]"""
    ld = np.longdouble
    k = kmax(N, M, span)
    K = 2 * k + 1
    s, o, n = ld(span) / ld(M), np.fmod(ld(origin), ld(N)), ld(N)
    pi = ld("3.141592653589793238462643383279502884")

    def e(x):                                                          # exp(i pi x), x reduced modulo 2 first
        r = np.fmod(x, ld(2))
        return np.cos(pi * r) + 1j * np.sin(pi * r)

    j = np.arange(K).astype(ld)
    g = np.where(2 * np.abs(np.arange(K) - k) == N, ld(0.5), ld(1))
    pre = g * e(np.fmod(2 * (j - k) * o / n, ld(2)) + np.fmod(s * j * j / n, ld(2)))
    m = np.arange(M).astype(ld)
    post = (s / n) * e(np.fmod(s * m * m / n, ld(2)) - np.fmod(2 * k * m * s / n, ld(2)))
    d = np.arange(-(K - 1), M).astype(ld)
    c = e(-np.fmod(s * d * d / n, ld(2)))
    return k, pre, post, c


def view_1d_chirp(x, M, origin, span):
    """the amplitude-preserving y through the chirp-z factorisation (direct convolution), for the comparison with view_1d"""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    k, pre, post, c = chirp_tables(N, M, origin, span)
    K = 2 * k + 1
    X = np.fft.fft(x)
    Z = X[(np.arange(K) - k) % N] * pre.astype(np.complex128)
    c = c.astype(np.complex128)
    y = np.array([np.sum(Z * c[(m - np.arange(K)) + (K - 1)]) for m in range(M)])
    return y * post.astype(np.complex128) * (M / float(span))
