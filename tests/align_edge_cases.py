"""The edges of the aligner's geometry (csrc/plan_rules.cpp, align_geometry): the literal table of windows, bands, fine grids and
decimations that tests/test_gpu_align_edges.py runs the five kernels of csrc/kernels_align.hpp at, the forty-five pairs of its
long call, and the bars.  Test infrastructure only: no test lives here and nothing needs a device; tests/test_align_edge_oracle.py
proves on the fp64 oracle (tests/align_oracle.py) alone every condition the GPU tests rest on, and recomputes every literal below
(the complex64 figures within a factor of three: they are samples of rounding noise and move with the machine's matrix product).

Bars.  None is taken from the code under test.
    peak, peak_coarse: EDGE_PEAK_BAR, four times the largest difference in peak or peak_coarse between the oracle in complex64 and
        the oracle in complex128 over the rows of the table and the three input formats (the rule of tests/test_gpu_align.py's
        PEAK_BAR, on these rows).
    dx, dy, every pair: one fine cell, d / kappa (tests/test_gpu_align.py has the reason).
    dx, dy, the pairs that qualify: 4 d max(f, 2e-6) input pixels, f the row's own largest complex64-vs-complex128 difference of dx or
        dy in decimated pixels (column `shift_c64` of the table), floored at 2e-6 so that a row with a lucky small figure gets no bar
        below fp32 noise.  The factor 4 is the one the project gives fp32 over the oracle's own fp32 restatement.  A pair qualifies
        when the ORACLE's two vertex deltas are within 0.49 of a fine cell: beyond that the fine argmax sits on a near-tie of two
        cells, which fp32 may settle the other way, and the two parabolas through different triples of points differ by far more
        than rounding -- such a pair has the hard bar alone.  The cap (tests/test_align_edge_oracle.py): at least 5 of every 7
        pairs of a row and format qualify (a row with fewer pairs may lose one), and at least 90 % of all.

Seeds.  Per row the first seed of 0..SEED_RANGE-1, among those whose pairs meet the cap just stated, whose smallest gap between the
oracle's best and second-best coarse value, over the row's shifts and the three input formats, is the largest (the rule of
align_oracle.CASE_SEED, with the cap as a side condition).  The gap stands beside each seed."""
import numpy as np

import align_oracle as AO

SEED_RANGE = 100
TIGHT_DELTA = 0.49           # a pair qualifies for the tight bar when the oracle's |dx_| and |dy_| are at most this
SHIFT_FLOOR = 2e-6           # decimated pixels
FORMATS = {"rgb8": lambda f: f,
           "planar_f32": lambda f: AO.planes_of(f, np.float32),
           "planar_f16": lambda f: AO.planes_of(f, np.float16)}

FAR_SHIFTS = [(-30.3, 15.6), (40.25, -20.75)]
MIN16_SHIFTS = [(0.0, 0.0), (1.25, -0.5), (-0.8, 0.6), (0.37, 0.81)]

# (name, W, H, window, d, band, upsample, shifts in decimated pixels, clip seed, shift_c64)   -- smallest oracle gap of the seed
ROWS = (
    ("min16", 24, 20, (16, 16), 1, 0.5, 32, MIN16_SHIFTS, 83, 3.97e-06),    # 7.1e-2
    ("tall", 40, 144, (32, 128), 1, 0.5, 32, AO.SHIFTS, 43, 1.18e-05),    # 5.6e-3
    ("band1", 80, 48, (64, 32), 1, 1.0, 32, AO.SHIFTS, 42, 1.91e-06),    # 2.4e-2
    ("band099", 80, 48, (64, 32), 1, 0.99, 32, AO.SHIFTS, 56, 2.96e-06),    # 1.7e-2
    ("band01", 80, 48, (64, 32), 1, 0.1, 32, AO.WIDE_SHIFTS, 48, 0.00015),    # 3.6e-3
    ("band025", 144, 80, (128, 64), 1, 0.25, 32, AO.WIDE_SHIFTS, 57, 2.25e-05),    # 2.8e-2
    ("k4", 80, 48, (64, 32), 1, 0.5, 4, AO.SHIFTS, 24, 2.36e-06),    # 1.1e-2
    ("k64", 80, 48, (64, 32), 1, 0.5, 64, AO.SHIFTS, 24, 1.03e-05),    # 1.1e-2
    ("d4", 272, 140, (64, 32), 4, 0.5, 32, AO.SHIFTS, 11, 5.99e-06),    # 1.1e-2
    ("d8", 280, 150, (32, 16), 8, 0.5, 32, AO.SHIFTS[:4], 94, 3.76e-06),    # 1.2e-1
    ("x1024", 1040, 40, (1024, 32), 1, 0.5, 32, AO.WIDE_SHIFTS, 10, 3.2e-05),    # 7.7e-2
    ("y1024", 40, 1040, (32, 1024), 1, 0.5, 32, AO.WIDE_SHIFTS, 5, 2.53e-05),    # 1.0e-1
    ("far", 144, 80, (128, 64), 1, 0.5, 32, FAR_SHIFTS, 68, 5.57e-06),    # 4.2e-2
)
NAMES = [r[0] for r in ROWS]
# four times the largest complex64-vs-complex128 difference of peak or peak_coarse over ROWS and FORMATS
EDGE_PEAK_C64 = 3.13e-07
EDGE_PEAK_BAR = 4 * EDGE_PEAK_C64
# rows whose K is too small for the oracle to be held to the truth: they only have to match the oracle
NOT_HELD_TO_THE_TRUTH = ("band01", "d8")


def row(name):
    return ROWS[NAMES.index(name)]


def geometry(r):
    return AO.geometry(r[1], r[2], r[3], r[4], r[5], r[6])


def tight_bar(r):
    """input pixels"""
    return 4.0 * r[4] * max(r[9], SHIFT_FLOOR)


def qualifies(o):
    return abs(o["dx_"]) <= TIGHT_DELTA and abs(o["dy_"]) <= TIGHT_DELTA


def row_clip(r, seed=None):
    """(reference frame, the moved frames, their true shifts in input pixels), read-only"""
    d = r[4]
    true = [(sx * d, sy * d) for (sx, sy) in r[7]]
    frames = AO.clip(r[1], r[2], d, [(0.0, 0.0)] + true, r[8] if seed is None else seed)
    for f in frames:
        f.flags.writeable = False
    return frames[0], frames[1:], true


def figures(oracle, single, d):
    """(largest |peak| or |peak_coarse| difference, largest |dx| or |dy| difference in decimated pixels) between two lists of
    estimates of the same pairs"""
    dp = max(max(abs(a["peak"] - b["peak"]), abs(a["peak_coarse"] - b["peak_coarse"])) for a, b in zip(oracle, single))
    ds = max(max(abs(a["dx"] - b["dx"]), abs(a["dy"] - b["dy"])) for a, b in zip(oracle, single)) / d
    return dp, ds


# ------------------------------------------------------------------------------------------------------------ the forty-five pairs
# the eight frames of AO.CASES[0] (the reference and its seven moved frames), every ordered pair (a, b), a != b, in row-major order:
# frame 0 is the reference of pairs 0..6 and the current frame of pairs 7, 14, 21, 28, 35 and 42; the first 45 of the 56
LONG_CASE = AO.CASES[0]
LONG_PAIRS = [(a, b) for a in range(8) for b in range(8) if a != b][:45]
LONG_MAX_BATCH = 40          # one chunk of 40 pairs -- row launches of 16, 16 and 8 -- and a second chunk of 5


def long_frames():
    ref, moved, _ = AO.case_clip(*LONG_CASE[:2], LONG_CASE[3])
    frames = [ref] + moved
    for f in frames:
        f.flags.writeable = False
    return frames


# ------------------------------------------------------------------------------------------------------------------- no signal
# The rows of the no-signal test: AO.CASES[0] (d = 1) and the d4 row.  A black frame's windowed luma is identically zero, so
# P[0,0] -- the product of the two frames' sums -- is exactly 0 and step 3 (include/fftup.h) keeps no bin: R = 0 and r = 0 everywhere,
# both argmaxes are decided by the tie rule alone (lowest row-major index) -- coarse cell (0, 0), fine cell (0, 0), which is the
# offset -1 on both axes, no parabola at the fine grid's border -- and the result is dx = dy = -d, peak = peak_coarse = 0.
NO_SIGNAL_ROWS = ("case0", "d4")


def no_signal_case(name):
    """(W, H, window, d, band, upsample, reference frame, an ordinary moved frame, a black frame)"""
    if name == "case0":
        W, H, window, d = AO.CASES[0]
        ref, moved, _ = AO.case_clip(W, H, d)
        band, kappa, cur = 0.5, 32, moved[1]
    else:
        r = row(name)
        W, H, window, d, band, kappa = r[1:7]
        ref, moved, _ = row_clip(r)
        cur = moved[1]
    return W, H, window, d, band, kappa, ref, cur, np.zeros_like(ref)


def dead_result(d):
    return (-float(d), -float(d), 0.0, 0.0)
