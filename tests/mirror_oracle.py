"""fp64 oracle of the mirror view plans (fftup_plan_create_view with FFTUP_FLAG_MIRROR, include/fftup.h).  numpy only.

Per axis, separable: input x[n] (n < N), an output of M points, a view (origin, span), step s = span / M, output pixel m at
t_m = origin + m s.  The frame is continued by its half-sample even reflection, x~[n] = x[n] (n < N), x~[n] = x[2N-1-n]
(N <= n < 2N), period 2N, and the plan evaluates the view formula (tests/view_oracle.py) of x~.  In closed form
    C[k]  = sum_n x[n] cos(pi k (2n+1) / 2N)                         (DCT-II, k = 0 .. N-1)
    kmax  = min(N - 1, floor((double)(N M) / max(span, (double)M)))
    y[m]  = C[0]/N + (2/N) sum_{k=1..kmax} C[k] cos(pi k (2 t_m + 1) / 2N)
(bin N of the extension is identically zero: the cap at N - 1 changes nothing).  The pre-sharpen image is
R = y span_x span_y / (uW uH); the sharpen pass takes the view plans' effective factor (view_oracle.effective_factor).

The kernels (csrc/kernels_mirror.hpp) reach C through a transform of length N, not 2N: the reordering identities below.
"""
import numpy as np

import view_oracle as V


def kmax(N, M, span):
    """the last cosine kept, in double exactly as the header writes it (N M is exact, the quotient correctly rounded)"""
    return int(min(N - 1, np.floor(float(N * M) / max(float(span), float(M)))))


def table_kmax(N, M, span):
    """what the plan reports and its tables are sized by (csrc/mirror_tables.hpp): the view rule of the doubled period,
    min(N, floor(N M / max(span, M))) -- N itself only as the zero bin, so the cosines kept stop at kmax() above"""
    return V.kmax(2 * N, M, span)


def conv_length(N, M):
    """the convolution length of a mirror axis: the smallest 2,3,5,7-smooth L >= 2N + M"""
    return V.smooth_from(2 * N + M)


def mirror_factors(N, M, origin, span):
    """the two factors of the cosine form, A = E D: D [kmax + 1][N] the DCT-II's rows, E [M][kmax + 1] the cosines at the positions
    (for lengths of thousands: E (D x) in place of forming A)"""
    k = np.arange(kmax(N, M, span) + 1)
    t = V.positions(M, origin, span)
    g = np.where(k == 0, 1.0, 2.0) / N
    E = np.cos(np.pi * np.outer(2 * t + 1, k) / (2 * N)) * g                   # [M][kmax + 1]
    D = np.cos(np.pi * np.outer(k, 2 * np.arange(N) + 1) / (2 * N))            # [kmax + 1][N]: the DCT-II
    return E, D


def mirror_matrix(N, M, origin, span):
    """y = A x, A [M][N] real: the cosine form"""
    E, D = mirror_factors(N, M, origin, span)
    return E @ D


def chirp_tables(N, M, origin, span):
    """the chirp-z factorisation the kernels run (csrc/mirror_tables.hpp) in longdouble: the periodic view's tables
    (view_oracle.chirp_tables) of the period 2N aimed at origin + 1/2, the sum formed in longdouble (exact)"""
    return V.chirp_tables(2 * N, M, np.longdouble(origin) + np.longdouble(0.5), span)


def mirror_1d_chirp(x, M, origin, span):
    """the amplitude-preserving y through that factorisation (direct convolution), Z_j = 2 C[|j - kmax|] with C[N] = 0: for the
    comparison with mirror_matrix"""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    k, pre, post, c = chirp_tables(N, M, origin, span)
    K = 2 * k + 1
    Cc = np.append(dct2(x), 0.0)
    Z = 2 * Cc[np.abs(np.arange(K) - k)] * pre.astype(np.complex128)
    c = c.astype(np.complex128)
    y = np.array([np.sum(Z * c[(m - np.arange(K)) + (K - 1)]) for m in range(M)])
    return y * post.astype(np.complex128) * (M / float(span))


def extend(x, axis=-1):
    """the half-sample even reflection: 2N points along `axis`"""
    x = np.asarray(x)
    return np.concatenate([x, np.flip(x, axis)], axis)


def mirror_matrix_ext(N, M, origin, span):
    """the same map as the periodic view matrix of the doubled period, its columns folded onto the N samples that exist"""
    Vm = V.view_matrix(2 * N, M, origin, span)                                 # complex, real up to rounding
    return Vm[:, :N] + Vm[:, ::-1][:, :N]                                      # x~[2N-1-n] = x[n]


def mirror_planes(planes, uW, uH, origin, span):
    """planes [C][H][W] -> the amplitude-preserving image y [C][uH][uW] (fp64); origin = (x, y), span = (x, y)"""
    planes = np.asarray(planes, dtype=np.float64)
    _, H, W = planes.shape
    return mirror_matrix(H, uH, origin[1], span[1]) @ planes @ mirror_matrix(W, uW, origin[0], span[0]).T


def mirror_R(planes, uW, uH, origin, span):
    """the pre-sharpen image R = y span_x span_y / (uW uH)"""
    return mirror_planes(planes, uW, uH, origin, span) * (float(span[0]) * float(span[1]) / (uW * uH))


def centre_origin(N, M):
    """the origin at which a view of span N is the DCT modes' lattice: output pixel m at (m + 1/2) N / M - 1/2"""
    return (N / M - 1) / 2


# ---- the DCT-II of N points through one DFT of N points
def dct2(x):
    """C[k] = sum_n x[n] cos(pi k (2n+1) / 2N), real or complex x, by the definition"""
    x = np.asarray(x)
    N = len(x)
    return np.cos(np.pi * np.outer(np.arange(N), 2 * np.arange(N) + 1) / (2 * N)) @ x


def reorder(x):
    """v[q] = x[2q] (q < ceil(N/2)), v[N-1-q] = x[2q+1] (q < floor(N/2))"""
    x = np.asarray(x)
    N = len(x)
    v = np.empty_like(x)
    v[:(N + 1) // 2] = x[0::2]
    v[N - 1 - np.arange(N // 2)] = x[1::2]
    return v


def dct2_reordered_real(x):
    """real x: C[k] = Re(w_k V[k]), C[N-k] = -Im(w_k V[k]) for k = 0 .. N/2 (floor), V = DFT_N(reorder(x)), w_k = exp(-i pi k / 2N)"""
    N = len(x)
    Vv = np.fft.fft(reorder(np.asarray(x, dtype=np.float64)))
    k = np.arange(N // 2 + 1)
    wV = np.exp(-1j * np.pi * k / (2 * N)) * Vv[k]
    Cc = np.empty(N)
    Cc[k] = wV.real
    Cc[N - k[1:]] = -wV.imag[1:]
    return Cc


def dct2_reordered_complex(z):
    """complex z: C[0] = V[0], C[k] = (w_k V[k] + conj(w_k) V[N-k]) / 2"""
    N = len(z)
    Vv = np.fft.fft(reorder(np.asarray(z, dtype=np.complex128)))
    k = np.arange(N)
    w = np.exp(-1j * np.pi * k / (2 * N))
    return (w * Vv + np.conj(w) * Vv[(N - k) % N]) / 2
