"""Shift estimates (fftup_align_shifts, include/fftup.h) restated in numpy: the geometry rules, steps 1-6 of the estimate in fp64 (or,
for the tolerance of the peak values, in complex64), and the synthetic clips the tests run on.

The clips are 8-bit on purpose: quantisation puts a broadband floor far above fp32 rounding into every bin of the band, so the unit
phasors R = P / |P| of the library and of this file agree instead of being two unrelated noise phases."""
import numpy as np

LUMA = (0.2126, 0.7152, 0.0722)


def _pow2_floor(v):
    p = 1
    while p * 2 <= v:
        p *= 2
    return p


def geometry(W, H, window=None, decimate=0, band=0.0, upsample=0):
    """the decisions of fftup_align_create for a valid request (the library's own rules: csrc/plan_rules.cpp, align_geometry)"""
    d = decimate
    if not d:
        d = next((q for q in (1, 2, 4, 8) if _pow2_floor(W // q) <= 1024 and _pow2_floor(H // q) <= 1024), 8)
    nx, ny = window if window else (min(1024, _pow2_floor(W // d)), min(1024, _pow2_floor(H // d)))
    assert nx * d <= W and ny * d <= H and W // d >= 16 and H // d >= 16
    b = float(np.float32(band)) if band else 0.5
    g = dict(W=W, H=H, d=d, nx=nx, ny=ny, crop_x=(W - nx * d) // 2, crop_y=(H - ny * d) // 2, kappa=upsample or 32,
             band_kx=int(np.floor(b * nx / 2)), band_ky=int(np.floor(b * ny / 2)))
    return g


def luma_planes(frame):
    """fp64 luma [H][W] of an 8-bit frame [H][W][3] (code / 255) or of planes [3][H][W] (the stored values)"""
    f = np.asarray(frame)
    if f.dtype == np.uint8:
        f = np.transpose(f, (2, 0, 1)).astype(np.float64) / 255.0
    f = f.astype(np.float64)
    return LUMA[0] * f[0] + LUMA[1] * f[1] + LUMA[2] * f[2]


def windowed(frame, g):
    """step 1: luma, d x d box mean, centred crop, separable window"""
    d, nx, ny = g["d"], g["nx"], g["ny"]
    y = luma_planes(frame)[g["crop_y"]:g["crop_y"] + ny * d, g["crop_x"]:g["crop_x"] + nx * d]
    y = y.reshape(ny, d, nx, d).mean(axis=(1, 3))
    wx = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(nx) + 0.5) / nx)
    wy = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(ny) + 0.5) / ny)
    return y * wy[:, None] * wx[None, :]


def _signed(n):
    k = np.arange(n)
    return np.where(k < n - k, k, k - n)          # [-n/2, n/2)


def estimate(ref, cur, g, single=False):
    """steps 1-6 for one pair -> dict(dx, dy, peak, peak_coarse, coarse=(p_x, p_y), fine=(i, j), dx_, dy_, K, gap, near): gap is the
    difference between the best and the second-best coarse value, in peak_coarse units; near: the coarse values within 1e-3 of the best,
    itself included; dx_, dy_: the parabola's vertex per axis, in fine cells from the fine maximum, in [-0.5, 0.5]; K: the bins of the
    band.  single: complex64 / float32 arithmetic from step 2 on"""
    ct, ft = (np.complex64, np.float32) if single else (np.complex128, np.float64)
    nx, ny, d, kappa = g["nx"], g["ny"], g["d"], g["kappa"]
    a, b = windowed(ref, g).astype(ft), windowed(cur, g).astype(ft)
    # 2. one complex transform, separated
    Z = np.fft.fft2((a + 1j * b).astype(ct)).astype(ct)
    Zm = np.conj(np.roll(Z[::-1, ::-1], (1, 1), axis=(0, 1)))          # conj Z[-k]
    A, B = (Z + Zm) / ft(2), (Z - Zm) / ct(2j)
    # 3. cross-power, band, floor
    P = (B * np.conj(A)).astype(ct)
    mag = np.abs(P)
    sx, sy = _signed(nx), _signed(ny)
    band = (np.abs(sy)[:, None] <= g["band_ky"]) & (np.abs(sx)[None, :] <= g["band_kx"])
    K = int(band.sum())
    keep = band & (mag > ft(1e-9) * mag[0, 0]) & (mag[0, 0] > 0)          # (P[0,0] = 0, a black frame: no bin carries signal)
    R = np.zeros_like(P)
    R[keep] = P[keep] / mag[keep]
    # 4. coarse peak
    r = np.real(np.fft.ifft2(R)).astype(ft)
    flat = r.ravel()
    order = np.argsort(-flat, kind="stable")
    p = int(order[0])
    py, px = divmod(p, nx)
    scale = ft(nx * ny) / ft(K)
    # 5. fine peak: the trigonometric interpolant on (2 kappa + 1)^2 points, two small products
    off = np.arange(-kappa, kappa + 1) / kappa
    kx, ky = np.sort(sx[np.abs(sx) <= g["band_kx"]]), np.sort(sy[np.abs(sy) <= g["band_ky"]])
    Ex = np.exp(2j * np.pi * kx[:, None] * (px + off)[None, :] / nx).astype(ct)
    Ey = np.exp(2j * np.pi * ky[:, None] * (py + off)[None, :] / ny).astype(ct)
    Rb = R[np.ix_(ky % ny, kx % nx)]
    F = (np.real(Ey.T @ (Rb @ Ex)) / ft(nx * ny)).astype(ft)          # F[j][i]
    q = int(np.argmax(F.ravel()))                                     # (the first of equal maxima: lowest row-major index)
    j, i = divmod(q, 2 * kappa + 1)

    def vertex(lo, mid, hi):
        den = lo - 2 * mid + hi
        return 0.5 * (lo - hi) / den if den != 0 else 0.0

    dx_ = vertex(F[j, i - 1], F[j, i], F[j, i + 1]) if 0 < i < 2 * kappa else 0.0
    dy_ = vertex(F[j - 1, i], F[j, i], F[j + 1, i]) if 0 < j < 2 * kappa else 0.0
    # 6. result
    s_x = px + (i - kappa + dx_) / kappa
    s_y = py + (j - kappa + dy_) / kappa
    s_x -= nx * np.floor((s_x + nx / 2) / nx)
    s_y -= ny * np.floor((s_y + ny / 2) / ny)
    return dict(dx=float(d * s_x), dy=float(d * s_y), peak=float(F[j, i] * scale), peak_coarse=float(flat[p] * scale),
                coarse=(px, py), fine=(i, j), dx_=float(dx_), dy_=float(dy_), K=K, gap=float((flat[order[0]] - flat[order[1]]) * scale),
                near=[float(flat[q] * scale) for q in order[:8] if (flat[order[0]] - flat[q]) * scale <= 1e-3])


def clip(W, H, d, shifts, seed=0):
    """8-bit frames [H][W][3] of one moving scene: frame i is the scene shifted by shifts[i] = (dx, dy) input pixels, frame(x, y) =
    scene(x - dx, y - dy).  Per channel a random field with the Gaussian spectrum exp(-|f|^2 / c^2), c = 0.35 / d cycles per pixel, on
    a periodic canvas of 2H x 2W; shifted by an exact Fourier phase ramp, normalised to [0, 1] (one affine map per channel for the
    whole clip, from the unshifted field), cropped to the top-left H x W and rounded to 8 bits."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ch, cw = 2 * H, 2 * W
    fy, fx = np.fft.fftfreq(ch)[:, None], np.fft.fftfreq(cw)[None, :]
    c = 0.35 / d
    amp = np.exp(-(fx * fx + fy * fy) / (c * c))
    frames = [np.empty((H, W, 3), np.uint8) for _ in shifts]
    for k in range(3):
        S = np.fft.fft2(rng.standard_normal((ch, cw))) * amp
        base = np.real(np.fft.ifft2(S))
        lo, hi = base.min(), base.max()
        for n, (dx, dy) in enumerate(shifts):
            f = np.real(np.fft.ifft2(S * np.exp(-2j * np.pi * (fx * dx + fy * dy))))
            f = np.clip((f - lo) / (hi - lo), 0.0, 1.0)
            frames[n][:, :, k] = np.rint(255.0 * f[:H, :W]).astype(np.uint8)
    return frames


def planes_of(rgb, dtype):
    """the PLANAR form of an 8-bit frame: [3][H][W] of code / 255 in `dtype`"""
    return (np.transpose(rgb, (2, 0, 1)).astype(np.float64) / 255.0).astype(dtype)


# what the tests of the estimate run on: (W, H, window, d), and the shifts in decimated pixels (each is multiplied by d)
CASES = [(80, 48, (64, 32), 1), (160, 96, (64, 32), 2), (144, 80, (128, 64), 1)]
SHIFTS = [(0.0, 0.0), (3.25, -1.5), (-2.4, 2.3), (0.37, 0.81), (-0.5, -0.5), (4.0, -3.0), (-3.7, 1.2)]
# ... and the GPU parity test's fourth: three radix-8 stages on x, a window that is not square.  Its shifts are SHIFTS with the half-pixel
# components moved to quarter pixels.  A shift of half a pixel puts the correlation peak midway between two grid cells: their values
# differ only by what quantisation and the moved crop leave, which shrinks with the square root of the window's pixel count -- about
# 5e-3 of the peak at 64 x 32, 2e-3 at 128 x 64 and 4e-4 at 512 x 256, where none of 400 clip seeds brings (3.25, -1.5) and
# (-0.5, -0.5) above the 1e-3 the parity test requires of the ORACLE before it compares coarse cells.  The three smaller cases keep
# the half-pixel shifts (and meet the 1e-3); at 512 x 256 the same two shifts run in a test of their own, WIDE_HALF_SHIFTS, which
# accepts either of the tied cells.
WIDE_CASE = (600, 300, (512, 256), 1)
WIDE_SHIFTS = [(0.0, 0.0), (3.25, -1.25), (-2.4, 2.3), (0.37, 0.81), (-0.25, -0.75), (4.0, -3.0), (-3.7, 1.2)]
WIDE_HALF_SHIFTS = [(3.25, -1.5), (-0.5, -0.5)]
# The clip's seed per case, judged on THIS file's fp64 estimate alone: the first of 0..399 whose smallest gap between the best and the
# second-best coarse value, over the seven shifts and the three input formats (8-bit, float and half planes), is the largest --
# 4.5e-3, 3.1e-3, 2.4e-3 of the peak.  (The wide case's shifts have no near-ties: its seed is the one of the half-pixel search.)
CASE_SEED = {(80, 48): 1, (160, 96): 0, (144, 80): 37, (600, 300): 200}


def case_clip(W, H, d):
    """(reference frame, the moved frames, their true shifts in input pixels): the clip of one case -- seven moved frames; the wide
    case has two more, the half-pixel shifts WIDE_HALF_SHIFTS"""
    shifts = WIDE_SHIFTS + WIDE_HALF_SHIFTS if (W, H) == WIDE_CASE[:2] else SHIFTS
    true = [(sx * d, sy * d) for (sx, sy) in shifts]
    frames = clip(W, H, d, [(0.0, 0.0)] + true, CASE_SEED[(W, H)])
    return frames[0], frames[1:], true
