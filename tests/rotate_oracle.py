"""Rotation by three shears (include/fftup.h, fftup_rotate_frames) restated in numpy: the definition the kernels are held to.
`ctype` = np.complex128 is the oracle; np.complex64 runs the same code in single precision (numpy's pocketfft transforms a
complex64 array in single precision), which is where the fp32 bars of tests/test_gpu_rotate.py come from.  The phases are formed
and reduced in double for both, as the kernels do (csrc/rotate_phase.hpp)."""
import numpy as np

# (W, H): the shapes of the GPU tests -- the smallest at which each mechanism can go wrong
CASES = [
    (64, 32),        # powers of two, a Nyquist bin on both axes
    (60, 42),        # radices 3, 5 and 7, even
    (45, 21),        # odd: no Nyquist bin; W is no multiple of any column tile
    (96, 80),
    (4096, 16),      # the LDS limit of the row kernel, the other axis tiny
    (16, 4096),      # ... and of the column kernel
    (30, 1080),      # a real column length with a two-column last tile
]
ANGLES = [0.0, 0.02, -0.3, 0.7, -np.pi / 2]


def centre_of(W, H):
    return ((W - 1) / 2.0, (H - 1) / 2.0)


def factors(n, delta, ctype=np.complex128):
    """[line, bin]: bin k of a line of n points moved by delta[line] pixels is multiplied by exp(-2 pi i f delta / n), f the signed
    frequency; the Nyquist bin of an even n by cos(pi delta)"""
    delta = np.asarray(delta, dtype=np.float64)
    k = np.arange(n)
    f = np.where(2 * k < n, k, k - n).astype(np.float64)
    t = f[None, :] * delta[:, None] / float(n)
    r = t - np.rint(t)                                        # in [-1/2, 1/2]: exact
    w = np.exp(-2j * np.pi * r)
    w[r == 0.0] = 1.0
    if n % 2 == 0:
        w[:, n // 2] = np.cos(np.pi * (delta - 2.0 * np.rint(0.5 * delta)))
    return w.astype(ctype)


def shear(img, axis, coeff, centre, ctype=np.complex128):
    """img [..., H, W] real.  axis 'x': row y moves by coeff (y - centre) pixels; axis 'y': column x moves by coeff (x - centre)"""
    ft = np.float32 if ctype == np.complex64 else np.float64
    img = np.asarray(img, dtype=ft)
    H, W = img.shape[-2:]
    if axis == "x":
        w = factors(W, coeff * (np.arange(H, dtype=np.float64) - centre), ctype)            # [y, k]
        X = np.fft.fft(img.astype(ctype), axis=-1)
        return np.real(np.fft.ifft((X * w).astype(ctype), axis=-1)).astype(ft)
    w = factors(H, coeff * (np.arange(W, dtype=np.float64) - centre), ctype).T              # [k, x]
    X = np.fft.fft(img.astype(ctype), axis=-2)
    return np.real(np.fft.ifft((X * w).astype(ctype), axis=-2)).astype(ft)


def rotate(img, angle, centre=None, ctype=np.complex128):
    """out = x-shear(a) of y-shear(b) of x-shear(a) of img, a = -tan(angle / 2), b = sin(angle): content moves by
    [[cos, -sin], [sin, cos]] about the centre, out(p) ~ img(c + R(-angle)(p - c))"""
    H, W = np.asarray(img).shape[-2:]
    cx, cy = centre_of(W, H) if centre is None else centre
    a, b = -np.tan(0.5 * float(angle)), np.sin(float(angle))
    t = shear(img, "x", a, cy, ctype)
    t = shear(t, "y", b, cx, ctype)
    return shear(t, "x", a, cy, ctype)


def to_u8(x):
    """the rotator's 8-bit store: round to nearest"""
    return np.clip(np.floor(255.0 * np.asarray(x, dtype=np.float64) + 0.5), 0, 255).astype(np.uint8)


def noise_u8(W, H, seed):
    """8-bit uniform noise, [H, W, 3]"""
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def planes_of(rgb):
    """[H, W, 3] codes -> [3, H, W] values code / 255"""
    return np.ascontiguousarray(np.transpose(rgb, (2, 0, 1))).astype(np.float64) / 255.0


def gaussian(W, H, centre, offset=(8.0, -5.0), angle=0.0):
    """exp(-(u^2 / 18 + v^2 / 8)) centred at centre + R(angle) offset, its axes turned by `angle`: the analytic rotation of the
    angle = 0 Gaussian about `centre`"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    c, s = np.cos(angle), np.sin(angle)
    mx = centre[0] + c * offset[0] - s * offset[1]
    my = centre[1] + s * offset[0] + c * offset[1]
    dx, dy = x - mx, y - my
    u = c * dx + s * dy                                       # R(-angle) (p - m)
    v = -s * dx + c * dy
    return np.exp(-(u * u / 18.0 + v * v / 8.0))
