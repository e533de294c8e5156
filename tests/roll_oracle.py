"""Roll estimates (fftup_roll_angles, include/fftup.h) restated in numpy: the geometry rules, steps 1-7 of the estimate in fp64 (or,
for the fp32 bars of the GPU tests, in complex64 / float32), and the synthetic scenes the tests run on.

The scenes are 8-bit on purpose, as the aligner's clips: quantisation puts a broadband floor far above fp32 rounding into every bin,
so the log-magnitudes the library samples and the ones this file samples agree to rounding instead of being two unrelated noises."""
import numpy as np

import align_oracle as A


def _pow2_floor(v):
    p = 1
    while p * 2 <= v:
        p *= 2
    return p


def geometry(W, H, window=None, decimate=0, band=0.0, angles=0, upsample=0):
    """the decisions of fftup_roll_create for a valid request (the library's own rules: csrc/plan_rules.cpp, roll_geometry)"""
    d = decimate
    if not d:
        d = next((q for q in (1, 2, 4, 8) if _pow2_floor(W // q) <= 512 and _pow2_floor(H // q) <= 512), 8)
    nx, ny = window if window else (min(512, _pow2_floor(W // d)), min(512, _pow2_floor(H // d)))
    assert nx * d <= W and ny * d <= H and nx >= 32 and ny >= 32
    b = float(np.float32(band)) if band else 0.5
    n = min(nx, ny)
    nt = angles or n
    rho_max = int(np.floor(b * n))
    return dict(W=W, H=H, d=d, nx=nx, ny=ny, crop_x=(W - nx * d) // 2, crop_y=(H - ny * d) // 2, kappa=upsample or 32, n=n, angles=nt,
                rho_max=rho_max, rho_min=max(2, rho_max // 4), mb=nt // 4, K=2 * (nt // 4))


def profiles(ref, cur, g, single=False):
    """steps 1-3 -> (L_A, L_B), each [rho_max - rho_min + 1][n_theta]"""
    ct, ft = (np.complex64, np.float32) if single else (np.complex128, np.float64)
    nx, ny, n, nt = g["nx"], g["ny"], g["n"], g["angles"]
    a, b = A.windowed(ref, g).astype(ft), A.windowed(cur, g).astype(ft)
    # 2. one complex transform of the zero-padded pair, separated
    z = np.zeros((2 * ny, 2 * nx), dtype=ct)
    z[:ny, :nx] = (a + 1j * b).astype(ct)
    Z = np.fft.fft2(z).astype(ct)
    Zm = np.conj(np.roll(Z[::-1, ::-1], (1, 1), axis=(0, 1)))          # conj Z[-k]
    MA = np.log1p(np.abs((Z + Zm) / ft(2))).astype(ft)
    MB = np.log1p(np.abs((Z - Zm) / ct(2j))).astype(ft)
    # 3. polar samples, bilinear; the unit vectors are formed in double and rounded once
    th = np.pi * np.arange(nt) / nt
    c, s = np.cos(th).astype(ft), np.sin(th).astype(ft)
    rho = np.arange(g["rho_min"], g["rho_max"] + 1).astype(ft)
    kx = (rho[:, None] * c[None, :]) * ft(nx // n)
    ky = (rho[:, None] * s[None, :]) * ft(ny // n)
    x0, y0 = np.floor(kx), np.floor(ky)
    fx, fy = (kx - x0).astype(ft), (ky - y0).astype(ft)
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb, ya, yb = x0 % (2 * nx), (x0 + 1) % (2 * nx), y0 % (2 * ny), (y0 + 1) % (2 * ny)

    def sample(M):
        top = M[ya, xa] + fx * (M[ya, xb] - M[ya, xa])
        bot = M[yb, xa] + fx * (M[yb, xb] - M[yb, xa])
        return (top + fy * (bot - top)).astype(ft)

    return sample(MA), sample(MB)


def estimate(ref, cur, g, single=False):
    """steps 1-7 for one pair -> dict(angle, peak, peak_coarse, coarse=p, fine=i, delta, gap, next_cells, floor_ratio): gap is the
    difference between the best and the second-best coarse value, in peak_coarse units; next_cells the coarse values of the two
    cells beside the best one, in the same units; floor_ratio the smallest |P[m]| of the band over the largest.  single: complex64 / float32 arithmetic from step 2 on (the fine sums stay in double, as in the library)"""
    ct, ft = (np.complex64, np.float32) if single else (np.complex128, np.float64)
    nt, kappa, mb, K = g["angles"], g["kappa"], g["mb"], g["K"]
    LA, LB = profiles(ref, cur, g, single)
    # 4. cross-power of the angular spectra, summed over the radii; phase only
    FA, FB = np.fft.fft(LA.astype(ct), axis=1).astype(ct), np.fft.fft(LB.astype(ct), axis=1).astype(ct)
    P = np.zeros(nt, dtype=ct)
    for q in range(FA.shape[0]):                                       # (one fixed order, as the library sums)
        P = (P + FB[q] * np.conj(FA[q])).astype(ct)
    m = np.arange(nt)
    sm = np.where(m < nt - m, m, m - nt)
    band = (np.abs(sm) >= 1) & (np.abs(sm) <= mb)
    mag = np.abs(P).astype(ft)
    top = mag[band].max()
    keep = band & (mag > ft(1e-9) * top) & (top > 0)
    R = np.zeros(nt, dtype=ct)
    R[keep] = P[keep] / mag[keep]
    # 5. coarse peak
    r = np.real(np.fft.ifft(R)).astype(ft)
    order = np.argsort(-r, kind="stable")
    p = int(order[0])
    scale = ft(nt) / ft(K)
    # 6. fine peak: the interpolant on 2 kappa + 1 points
    off = np.arange(-kappa, kappa + 1)
    ks = np.sort(sm[band])
    E = np.exp(2j * np.pi * ((ks[:, None] * (p * kappa + off)[None, :]) % (kappa * nt)) / (kappa * nt)).astype(ct)
    F = (np.real(R[ks % nt].astype(np.complex128) @ E.astype(np.complex128)) / nt).astype(ft)
    i = int(np.argmax(F))
    delta = 0.0
    if 0 < i < 2 * kappa:
        den = F[i - 1] - 2 * F[i] + F[i + 1]
        delta = float(ft(0.5) * (F[i - 1] - F[i + 1]) / den) if den != 0 else 0.0
    # 7. result
    s = ft(p) + (ft(i - kappa) + ft(delta)) / ft(kappa)
    s = s - ft(nt) * np.floor((s + ft(nt) / 2) / ft(nt))
    return dict(angle=float(ft(np.pi) * s / ft(nt)) if single else float(np.pi * s / nt), peak=float(F[i] * scale),
                peak_coarse=float(r[p] * scale), coarse=p, fine=i, delta=float(delta), gap=float((r[order[0]] - r[order[1]]) * scale),
                next_cells=(float(r[(p - 1) % nt] * scale), float(r[(p + 1) % nt] * scale)), floor_ratio=float(mag[band].min() / top) if top > 0 else 0.0)


# ---- scenes: Gaussian blobs, turned analytically about the frame centre and translated
def scene(W, H, d, poses, seed=0, blobs=120):
    """8-bit frames [H][W][3]: frame i shows the scene turned by poses[i] = (angle, tx, ty) about the frame centre c = ((W - 1) / 2,
    (H - 1) / 2) and then moved by (tx, ty) input pixels: frame(p) = scene0(c + R(-angle)(p - c - t)) with R(a) = [[cos a, -sin a],
    [sin a, cos a]], the rotator's sign (tests/rotate_oracle.py).  The scene: `blobs` anisotropic Gaussians per channel, centres
    uniform in a disc that covers the frame's corners, axes of d * (0.8 .. 2.5) pixels, on a grey of 0.1; every frame is divided by the
    one maximum of the angle-0 frame, clipped to [0, 1] and rounded to 8 bits."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    rad = 0.55 * np.hypot(W, H)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    par = []
    for k in range(3):
        r, phi = rad * np.sqrt(rng.random(blobs)), 2 * np.pi * rng.random(blobs)
        par.append((r * np.cos(phi), r * np.sin(phi), d * (0.8 + 1.7 * rng.random(blobs)), d * (0.8 + 1.7 * rng.random(blobs)),
                    np.pi * rng.random(blobs), 0.3 + 0.7 * rng.random(blobs)))

    def render(angle, tx, ty):
        c, s = np.cos(angle), np.sin(angle)
        px, py = x - cx - tx, y - cy - ty
        qx, qy = c * px + s * py, -s * px + c * py                       # R(-angle)(p - c - t)
        out = np.empty((3, H, W))
        for k, (mx, my, su, sv, ori, amp) in enumerate(par):
            f = np.full((H, W), 0.1)
            for j in range(blobs):
                co, so = np.cos(ori[j]), np.sin(ori[j])
                ux, uy = qx - mx[j], qy - my[j]
                u, v = co * ux + so * uy, -so * ux + co * uy
                f += amp[j] * np.exp(-0.5 * (u * u / su[j] ** 2 + v * v / sv[j] ** 2))
            out[k] = f
        return out

    top = render(0.0, 0.0, 0.0).max()
    return [np.rint(255.0 * np.clip(np.transpose(render(*p), (1, 2, 0)) / top, 0.0, 1.0)).astype(np.uint8) for p in poses]


ANGLES = [0.0, 0.004, -0.02, 0.05, -0.1, 0.2, -0.35]
# translations in decimated pixels (each is multiplied by d): none is an integer
MOVES = [(0.8, -1.4), (1.3, -0.7), (-2.4, 1.6), (0.45, 2.2), (-1.7, -1.1), (2.6, 0.35), (-0.6, -2.3)]
# (W, H, window, d): the cases of the accuracy test, and the bar each must meet in radians (tests/test_roll_oracle.py)
ACCURACY_CASES = [(160, 160, (128, 128), 1), (320, 192, (128, 64), 2), (600, 300, (512, 256), 1)]
ACCURACY_BAR = {(160, 160): 1e-3, (320, 192): 2e-3, (600, 300): 0.5e-3}
# ... and of the GPU parity test: the smallest window a wide frame leaves, then the three above
GPU_CASES = [(80, 48, (64, 32), 1)] + ACCURACY_CASES
# The scene's seed per case, judged on THIS file's fp64 estimate alone: the first of 0..11 whose largest error over the seven poses is
# the smallest (tests/test_roll_oracle.py records the search's figures)
CASE_SEED = {(80, 48): 5, (160, 160): 2, (320, 192): 7, (600, 300): 10}


def case_scene(W, H, d):
    """(reference frame, the turned and moved frames, their true angles): the scene of one case"""
    poses = [(0.0, 0.0, 0.0)] + [(a, d * tx, d * ty) for a, (tx, ty) in zip(ANGLES, MOVES)]
    frames = scene(W, H, d, poses, CASE_SEED[(W, H)])
    return frames[0], frames[1:], list(ANGLES)
