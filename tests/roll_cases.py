"""What the GPU tests of the roll estimator (tests/test_gpu_roll.py, tests/test_gpu_rotate_angles.py) run on, and the bars they hold it
to -- shared with the CPU test that derives the bars (tests/test_roll_bars.py).  Per case of roll_oracle.GPU_CASES one reference frame
and SEVEN turned and moved frames (roll_oracle.case_scene), in three input formats; seven, so that an estimator with max_batch = 3
runs chunks of 3, 3 and 1.

The fp32 bars are not chosen and not typed in: bars() computes them, once per process, as four times the largest difference between
the oracle run in complex64 and the oracle run in complex128 over exactly these pairs and formats, the project's convention
(tests/rotate_cases.py, tests/test_gpu_align.py) -- the factor covers a different but equally valid order of fp32 operations."""
import functools

import numpy as np

import align_oracle as A
import roll_oracle as R

# name -> (precision of the estimator, conversion of an 8-bit frame to what the library reads)
FORMATS = {"rgb8": (0, lambda f: f),
           "planar_f32": (0, lambda f: A.planes_of(f, np.float32)),
           "planar_f16": (2, lambda f: A.planes_of(f, np.float16))}
CASE_IDS = ["%dx%d_w%dx%d_d%d" % (c[0], c[1], c[2][0], c[2][1], c[3]) for c in R.GPU_CASES]
GAP_FOR_SAME_CELL = 1e-3         # of the peak: below it the oracle's two best coarse cells are a coin toss in fp32


@functools.lru_cache(maxsize=None)
def scene(case):
    """(reference frame, the seven turned and moved frames, their true angles), 8-bit, read-only"""
    W, H, _, d = case
    ref, moved, true = R.case_scene(W, H, d)
    for f in [ref] + moved:
        f.flags.writeable = False
    return ref, tuple(moved), tuple(true)


@functools.lru_cache(maxsize=None)
def oracle(case, fmt, single=False):
    """the estimates of the case's seven pairs on the values the library reads in this format, in fp64 (single: complex64):
    computed once"""
    W, H, window, d = case
    conv = FORMATS[fmt][1]
    ref, moved, _ = scene(case)
    g = R.geometry(W, H, window, d)
    return tuple(R.estimate(conv(ref), conv(cur), g, single) for cur in moved)


@functools.lru_cache(maxsize=None)
def measured_c64():
    """per quantity the largest |complex64 oracle - complex128 oracle| over the GPU cases and formats, and whether the two ever
    disagreed on the coarse cell"""
    worst = dict(angle=0.0, peak=0.0, peak_coarse=0.0)
    same_cell = True
    for case in R.GPU_CASES:
        for fmt in FORMATS:
            for d, s in zip(oracle(case, fmt), oracle(case, fmt, True)):
                same_cell = same_cell and d["coarse"] == s["coarse"]
                for k in worst:
                    worst[k] = max(worst[k], abs(d[k] - s[k]))
    return worst, same_cell


def bars():
    """the fp32 bars of angle (radians), peak and peak_coarse: four times measured_c64()"""
    return {k: 4.0 * v for k, v in measured_c64()[0].items()}
