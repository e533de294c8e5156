"""What the GPU tests of the rotator (tests/test_gpu_rotate.py) run on, and the bars they hold it to -- shared with the CPU test that
keeps the bars honest (tests/test_rotate_bars.py).  Per shape of rotate_oracle.CASES one call of SEVEN frames of 8-bit uniform
noise: the five angles of rotate_oracle.ANGLES about the frame centre, one rotation about a centre off the frame's, and 0.7 again
on another frame -- seven, so that a rotator with max_batch = 3 runs chunks of 3, 3 and 1.

The fp32 bars are not chosen: they are four times the largest difference between the oracle run in complex64 and the oracle run
in complex128 over exactly these frames (float planes and 8-bit input alike), the project's convention (tests/test_gpu_align.py) --
the factor covers a different but equally valid order of fp32 operations.  Measured on the CPU (numpy 2.2, pocketfft):
    max |difference|  6.31e-7 (30 x 1080, half planes; 3.5e-7 .. 5.7e-7 elsewhere)   recorded as C64_MAX_ABS = 6.4e-7
    relative L2       2.03e-7 (60 x 42, 8-bit input; 1.3e-7 .. 1.9e-7 elsewhere)      recorded as C64_REL_L2  = 2.1e-7
so FP32_ABS = 2.56e-6 and FP32_REL_L2 = 8.4e-7.  tests/test_rotate_bars.py measures both again on every run and fails if either
recorded figure is no longer the measured one (above it, or below half of it)."""
import functools

import numpy as np

import rotate_oracle as R

C64_MAX_ABS = 6.4e-7
C64_REL_L2 = 2.1e-7
FP32_ABS = 4 * C64_MAX_ABS
FP32_REL_L2 = 4 * C64_REL_L2
NEAR_TIE_CAP = 0.01              # 8-bit output: at most this share of a frame may lie within 255 FP32_ABS of a rounding tie

N_FRAMES = 7


def rotations(W, H):
    """the seven (angle, c_x, c_y) of a shape"""
    cx, cy = R.centre_of(W, H)
    rots = [(a, cx, cy) for a in R.ANGLES]
    rots.append((0.25, W / 3.0, 2.0 * H / 3.0 + 0.5))
    rots.append((0.7, cx, cy))
    return rots


@functools.lru_cache(maxsize=None)
def frames_u8(W, H):
    """the seven frames of a shape, [7][H, W, 3] codes"""
    return tuple(R.noise_u8(W, H, 100 + i) for i in range(N_FRAMES))


def input_planes(W, H, kind):
    """the values a frame holds for the rotator, [7][3, H, W] float64: 'u8' code / 255, 'f32' / 'f16' that rounded to the type"""
    out = []
    for rgb in frames_u8(W, H):
        x = R.planes_of(rgb)
        if kind == "f32":
            x = x.astype(np.float32).astype(np.float64)
        elif kind == "f16":
            x = x.astype(np.float16).astype(np.float64)
        out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def oracle(W, H, kind, single=False):
    """the seven rotated frames of a shape in fp64 (single: the same code in complex64), [7][3, H, W] -- computed once, read-only"""
    ct = np.complex64 if single else np.complex128
    res = []
    for x, (a, cx, cy) in zip(input_planes(W, H, kind), rotations(W, H)):
        y = R.rotate(x, a, (cx, cy), ct).astype(np.float64)
        y.setflags(write=False)
        res.append(y)
    return tuple(res)


def near_tie(x):
    """where the 8-bit code of x is not decided within the fp32 bar: 255 x + 0.5 within 255 FP32_ABS of an integer"""
    v = 255.0 * x + 0.5
    return np.abs(v - np.rint(v)) <= 255.0 * FP32_ABS
