"""Case lists of the family sweeps (tests/test_host_family_sweep.py, tests/test_gpu_family_sweep.py): one deterministic generator per
arm -- exact (fftup_plan_create_size), odd (FFTUP_FLAG_ODD_SIZE), any (FFTUP_FLAG_ANY_SIZE, even lengths), down
(FFTUP_FLAG_DOWNSCALE, with and without FFTUP_FLAG_DCT), dct (FFTUP_FLAG_DCT upscale), view (fftup_plan_create_view).

Every list has two parts.  The FORCED strata are enumerated, not drawn: the shapes that look like edges from the code (lengths of 2
and 3, every parity class of an axis, a Nyquist bin that is folded or split, Bluestein lengths that are 2N - 1 itself, thin tall
frames at column tile widths 4, 2 and 1, a column pass just under the LDS limit, every residue of the spectrum's column count modulo
the tile width, views at the bounds of the step ...); they are the same under every seed.  The RANDOM fill tops the list up to
FFTUP_FAMILY_SWEEP_N cases (per arm; below, DEFAULT_N and BIG_N), drawn from FFTUP_SWEEP_SEED -- the knob and default of
tests/test_gpu_sweep.py -- plus an offset per arm.  Random input lengths stay at or below 200 per axis (the outputs of the arms with
a factor at or below 400); the only long axes are those of the thin frames, at most 16 pixels across.

Every case is a valid request: the arithmetic below mirrors the planner's (csrc/plan_rules.cpp) to place the strata, and
tests/test_host_family_sweep.py runs the planner itself over every case and names each stratum it must reach.  Plain module: numpy
only, no GPU, no pytest."""
import os

import numpy as np

ARMS = ("exact", "odd", "any", "down", "dct", "view")
OFFSET = {"exact": 101, "odd": 202, "any": 303, "down": 404, "dct": 505, "view": 606}
# the forced strata and a modest random part / a larger random part under FFTUP_BIG_TESTS=1
DEFAULT_N = {"exact": 64, "odd": 40, "any": 32, "down": 32, "dct": 24, "view": 36}
BIG_N = {"exact": 128, "odd": 72, "any": 72, "down": 72, "dct": 48, "view": 72}

ALIGN_CORNER, ALIGN_CENTRE = 0, 1
LDS_BYTES = 160 * 1024


def seed():
    return int(os.environ.get("FFTUP_SWEEP_SEED", "20260930"))


def count(arm):
    big = os.environ.get("FFTUP_BIG_TESTS", "0") != "0"
    return int(os.environ.get("FFTUP_FAMILY_SWEEP_N", (BIG_N if big else DEFAULT_N)[arm]))


# ---------------------------------------------------------------------------------- the planner's arithmetic (csrc/plan_rules.cpp)
def smooth(n):
    if n < 1:
        return False
    for q in (2, 3, 5, 7):
        while n % q == 0:
            n //= q
    return n == 1


def lpad(n):
    return n + (n >> 4) + 1


def two_buffers_fit(points):
    return 2 * 8 * lpad(points) <= LDS_BYTES


def bluestein_length(n, tk=1):
    L = 2 * n - 1
    while two_buffers_fit(L * tk):
        if smooth(L):
            return L
        L += 1
    return 0


def lds_length(n, tk):
    if not smooth(n):
        return bluestein_length(n, tk)
    return n if two_buffers_fit(n * tk) else 0


def bluestein_col_tk(H, uH):
    for tk in (8, 4, 2, 1):
        if lds_length(H, tk) and lds_length(uH, tk):
            return tk
    return 0


def conv_length(N, M):
    L = 2 * (N // 2) + M
    while not smooth(L):
        L += 1
    return L


def view_col_tk(H, uH):
    Ly = conv_length(H, uH)
    for tk in (8, 4, 2, 1):
        if lds_length(H, tk) and two_buffers_fit(max(lds_length(H, tk), Ly) * tk):
            return tk
    return 0


def out_size(n, u):
    """(uint32_t)(u n) in fp32, as fftup_plan_create computes it"""
    return int(np.float32(u) * np.float32(n))


def column_guard(u, uH):
    """the zero-padding range of the column pass, in fp32 as the planner computes it"""
    u, n, two, one = np.float32(u), np.float32(uH), np.float32(2), np.float32(1)
    return int(n / (two * u)), int((two * u - one) * n / (two * u))


def kmax(N, M, span):
    """the last bin a view keeps (include/fftup.h; tests/view_oracle.py)"""
    return int(min(N // 2, np.floor(float(N * M) / (2.0 * max(float(span), float(M))))))


def _bz_ok(*lengths):
    return all(smooth(n) or n <= 4096 for n in lengths)


SMOOTH_EVEN = [n for n in range(2, 201, 2) if smooth(n)]
SMOOTH_ANY = [n for n in range(2, 201) if smooth(n)]


def _fill(forced, arm, draw, n=None, s=None):
    """the forced strata, then cases drawn by `draw(rng)` (None: not a valid request, draw again) up to the arm's count; a count
    below the forced part never cuts a stratum"""
    rng = np.random.default_rng((seed() if s is None else s) + OFFSET[arm])
    out = list(forced)
    n = count(arm) if n is None else n
    while len(out) < n:
        c = draw(rng)
        if c is not None and c not in out:
            out.append(c)
    return out


# ------------------------------------------------------------------------------------------------------------------ arm `exact`
# (parity of N, parity of M, direction) of one axis: ten classes
AXIS_CLASSES = [("e", "e", "down"), ("e", "e", "up"), ("e", "o", "down"), ("e", "o", "up"), ("o", "e", "down"), ("o", "e", "up"),
                ("o", "o", "down"), ("o", "o", "up"), ("e", "e", "equal"), ("o", "o", "equal")]
_ROW_PAIRS = [(50, 32), (24, 40), (40, 25), (28, 45), (45, 36), (21, 64), (63, 35), (15, 27), (48, 48), (35, 35)]
_COL_PAIRS = [(36, 20), (30, 48), (32, 21), (20, 27), (49, 30), (25, 42), (45, 25), (9, 21), (20, 20), (21, 21)]


def axis_class(N, M):
    return ("o" if N & 1 else "e", "o" if M & 1 else "e", "down" if M < N else "up" if M > N else "equal")


def exact_valid(W, H, uW, uH, any_flag):
    if min(W, H, uW, uH) < 2 or 8 * uW < W or uW > 8 * W or 8 * uH < H or uH > 8 * H or W > 8192 or uW > 8192:
        return False
    if not all(smooth(n) for n in (W, H, uW, uH)) and not (any_flag and _bz_ok(W, H, uW, uH)):
        return False
    return bluestein_col_tk(H, uH) != 0


def exact_forced():
    out = []
    # every class of an axis on rows and on columns, at both alignments (50 -> 32 at the centres: a folded Nyquist bin under a phase
    # table; 24 -> 40: a split one)
    for a in (ALIGN_CORNER, ALIGN_CENTRE):
        for i in range(10):
            (W, uW), (H, uH) = _ROW_PAIRS[i], _COL_PAIRS[(i + 3) % 10]
            out.append((W, H, uW, uH, a, 0))
    # a length of 2 and a length of 3 in each of the four positions
    out += [(2, 2, 3, 3, ALIGN_CORNER, 0), (2, 2, 3, 3, ALIGN_CENTRE, 0), (3, 3, 2, 2, ALIGN_CENTRE, 0), (3, 2, 2, 3, ALIGN_CORNER, 0),
            (2, 3, 3, 2, ALIGN_CENTRE, 0), (2, 12, 16, 2, ALIGN_CENTRE, 0)]
    # single-stage lengths
    out += [(4, 5, 7, 8, ALIGN_CORNER, 0), (8, 7, 5, 4, ALIGN_CENTRE, 0)]
    # a non-smooth length in each position alone; all four non-smooth with four different Bluestein lengths (21, 25, 35, 40); the
    # Bluestein length is 2N - 1 itself for 11, 13, 23 and 41
    out += [(22, 20, 30, 24, ALIGN_CENTRE, 1), (20, 26, 30, 24, ALIGN_CORNER, 1), (20, 24, 34, 30, ALIGN_CENTRE, 1), (20, 24, 30, 38, ALIGN_CORNER, 1),
            (11, 13, 17, 19, ALIGN_CENTRE, 1), (11, 13, 13, 11, ALIGN_CORNER, 1), (41, 13, 23, 41, ALIGN_CENTRE, 1)]
    # min(W, uW) / 2 + 1 = 8, 9, 10, 11, 28, 13, 14, 15: every residue modulo the tile width 8 in the column kernels' last tile
    out += [(14, 6, 20, 10, ALIGN_CENTRE, 0), (24, 10, 16, 6, ALIGN_CORNER, 0), (18, 8, 25, 12, ALIGN_CENTRE, 0), (35, 12, 20, 9, ALIGN_CENTRE, 0),
            (54, 6, 64, 8, ALIGN_CORNER, 0), (36, 9, 24, 10, ALIGN_CENTRE, 0), (27, 10, 40, 6, ALIGN_CORNER, 0), (45, 8, 28, 12, ALIGN_CENTRE, 0)]
    # thin tall frames under the Bluestein rule: tile widths 4 (607: both column lengths, L = 1215), 2 (2003, L = 4032) and 1 (4093,
    # L = 8192); 1201 -> 700: a crop beside a Bluestein transform (L = 2401 at tile width 4), the column pass just under the LDS limit
    out += [(8, 607, 8, 607, ALIGN_CORNER, 1), (8, 2003, 8, 2003, ALIGN_CENTRE, 1), (16, 4093, 16, 4093, ALIGN_CORNER, 1), (8, 1201, 8, 700, ALIGN_CENTRE, 1)]
    return out


def exact_cases(n=None, s=None):
    def draw(rng):
        W, H = int(rng.integers(2, 201)), int(rng.integers(2, 201))
        uW = int(np.clip(round(W * 2.0 ** rng.uniform(-1.5, 1.5)), 2, 200)) if rng.random() > 0.15 else W
        uH = int(np.clip(round(H * 2.0 ** rng.uniform(-1.5, 1.5)), 2, 200)) if rng.random() > 0.15 else H
        any_flag = int(not all(smooth(x) for x in (W, H, uW, uH)))
        c = (W, H, uW, uH, int(rng.integers(0, 2)), any_flag)
        return c if exact_valid(W, H, uW, uH, any_flag) else None
    return _fill(exact_forced(), "exact", draw, n, s)


# -------------------------------------------------------------------------------------------------------------------- arm `odd`
# the factors with kernels specialised at plan time (README.md) and their reciprocals: what these plans take from cfg->upscale is the
# fp32 size rule (uint32_t)(u N) and the sharpen constant upsq
JIT_FACTORS = [1.125, 1.2, 1.25, 4 / 3, 1.4, 1.5, 1.6, 5 / 3, 1.75, 1.875, 2.0, 2.25, 2.5, 8 / 3, 3.0, 3.5, 4.0, 5.0, 6.0, 7.0, 8.0]


def _f32(u):
    return float(np.float32(u))


def odd_valid(W, H, u, extra):
    down = "down" in extra
    if down != (u < 1.0) or not (0.125 <= u < 1.0 if down else 1.0 <= u <= 64.0):
        return False
    uW, uH = out_size(W, u), out_size(H, u)
    if min(W, H, uW, uH) < 2 or not ((W | H | uW | uH) & 1) or W > 8192 or uW > 8192:
        return False
    if down and (uW >= W or uH >= H):
        return False
    if not down and (uW < W or uH < H):
        return False
    if not all(smooth(n) for n in (W, H, uW, uH)) and not ("any" in extra and _bz_ok(W, H, uW, uH)):
        return False
    return bluestein_col_tk(H, uH) != 0


def _odd_case(u, k, pool):
    """the k-th valid (W, H) of `pool` x `pool` for the factor u, in a fixed order"""
    down = u < 1.0
    found = []
    for W in pool:
        for H in pool:
            uW, uH = out_size(W, u), out_size(H, u)
            extra = ("any " if not all(smooth(n) for n in (W, H, uW, uH)) else "") + ("down" if down else "")
            if max(uW, uH) <= 200 and W != H and odd_valid(W, H, u, extra.strip()):
                found.append((W, H, u, extra.strip()))
    return found[(37 * k + 11) % len(found)]


def odd_forced():
    """every factor once, every second reciprocal once (the others come with the random fill): sizes from a fixed pool"""
    pool = [9, 10, 12, 15, 16, 18, 20, 21, 24, 25, 27, 30, 33, 35, 36, 39, 40, 45, 48, 50]
    out = [_odd_case(_f32(u), k, pool) for k, u in enumerate(JIT_FACTORS)]
    pool = [24, 27, 30, 35, 36, 40, 42, 45, 48, 55, 56, 60, 63, 64, 72, 75, 80, 81, 90, 96, 105, 120, 125, 135, 147, 160, 175, 189]
    out += [_odd_case(_f32(1.0 / u), k, pool) for k, u in enumerate(JIT_FACTORS[::2])]
    return out


def odd_cases(n=None, s=None):
    factors = [_f32(u) for u in JIT_FACTORS] + [_f32(1.0 / u) for u in JIT_FACTORS]

    def draw(rng):
        u = factors[int(rng.integers(0, len(factors)))]
        W, H = int(rng.integers(4, 201)), int(rng.integers(4, 201))
        uW, uH = out_size(W, u), out_size(H, u)
        extra = (("any " if not all(smooth(x) for x in (W, H, uW, uH)) else "") + ("down" if u < 1.0 else "")).strip()
        return (W, H, u, extra) if max(uW, uH) <= 400 and odd_valid(W, H, u, extra) else None
    return _fill(odd_forced(), "odd", draw, n, s)


# -------------------------------------------------------------------------------------------------------------------- arm `any`
ANY_UP = [1.0, 1.5, 2.0, 2.5, 3.0]
ANY_DOWN = [0.5, 0.25, 0.75]


def any_valid(W, H, u, down):
    if down != (u < 1.0) or not (0.125 <= u < 1.0 if down else 1.0 <= u <= 64.0):
        return False
    uW, uH = out_size(W, u), out_size(H, u)
    if min(W, H, uW, uH) < 2 or (W | H | uW | uH) & 1 or uW > 8192 or W > 8192:
        return False
    if not down and column_guard(u, uH) != (H // 2, uH - H // 2):                # the symmetric zero-padding range of the oracle's closed form
        return False
    if all(smooth(n) for n in (W, H, uW, uH)) or not _bz_ok(W, H, uW, uH):
        return False
    return bluestein_col_tk(H, uH) != 0


def any_forced():
    out = []
    # ncols = W/2 + 1 (an upscale) or uW/2 + 1 (a downscale) = 8 .. 15: every residue modulo the tile width; every factor; a non-smooth
    # length in every position (22 x 26 -u 1: all four; 14 x 38: H and uH only; 52 x 20 -u 0.5 -> 26 x 10: uW only)
    out += [(14, 38, 2.0, False), (16, 44, 1.5, False), (18, 46, 3.0, False), (20, 52, 2.5, False), (22, 26, 1.0, False), (24, 34, 2.0, False),
            (52, 20, 0.5, True), (28, 52, 1.5, False)]
    out += [(88, 40, 0.25, True), (40, 88, 0.75, True), (44, 40, 2.0, False), (40, 20, 1.1, False)]
    # thin tall frames under the Bluestein rule: tile widths 4, 2 and 1
    out += [(8, 302, 2.0, False), (16, 2006, 1.0, False), (8, 4094, 1.0, False), (8, 2428, 0.5, True)]
    return out


def any_cases(n=None, s=None):
    def draw(rng):
        down = rng.random() < 0.25
        u = float(rng.choice(ANY_DOWN if down else ANY_UP))
        W, H = 2 * int(rng.integers(2, 101)), 2 * int(rng.integers(2, 101))
        if max(out_size(W, u), out_size(H, u)) > 400:
            return None
        return (W, H, u, bool(down)) if any_valid(W, H, u, down) else None
    return _fill(any_forced(), "any", draw, n, s)


# ------------------------------------------------------------------------------------------------------------------- arm `down`
DOWN_FACTORS = [0.125, 0.25, 1 / 3, 0.4, 0.5, 0.6, 2 / 3, 0.75, 0.8, 0.875]


def down_valid(W, H, u, dct):
    uW, uH = out_size(W, u), out_size(H, u)
    return all(smooth(n) and n % 2 == 0 and n >= 2 for n in (W, H, uW, uH)) and uW < W and uH < H and W <= 8192


def down_forced():
    f = _f32
    # uW/2 + 1 = 8, 9, 10, 11, 28, 13, 22, 15: every residue modulo the tile width 8; with the next row every factor
    out = [(112, 48, f(0.125), False), (64, 24, f(0.25), False), (54, 36, f(1 / 3), False), (50, 40, f(0.4), False), (108, 60, f(0.5), False),
           (40, 20, f(0.6), False), (56, 40, f(0.75), False), (32, 16, f(0.875), False)]
    out += [(36, 24, f(2 / 3), False), (40, 20, f(0.8), False)]
    # an output length of 2 (both modes); the DCT downscale at a few factors
    out += [(16, 16, f(0.125), False), (4, 8, f(0.5), False), (16, 8, f(0.25), True), (4, 4, f(0.5), True), (96, 60, f(0.5), True), (40, 80, f(0.75), True),
            (60, 50, f(0.4), True), (54, 18, f(2 / 3), True)]
    return out


def down_cases(n=None, s=None):
    factors = [_f32(u) for u in DOWN_FACTORS]

    def draw(rng):
        u = factors[int(rng.integers(0, len(factors)))]
        W, H = int(rng.choice(SMOOTH_EVEN)), int(rng.choice(SMOOTH_EVEN))
        dct = bool(rng.random() < 0.3)
        return (W, H, u, dct) if down_valid(W, H, u, dct) else None
    return _fill(down_forced(), "down", draw, n, s)


# -------------------------------------------------------------------------------------------------------------------- arm `dct`
# tests/test_gpu_sweep.py: SMOOTH (the lengths up to 200 of it) and the factors of its _cases()
DCT_SMOOTH = [n for n in SMOOTH_EVEN if n >= 4]
DCT_FACTORS = [1.0, 1.25, 1.5, 2.0, 2.5, 3.0, 4.0]


def dct_valid(W, H, u):
    uW, uH = out_size(W, u), out_size(H, u)
    return W % 2 == 0 and H % 2 == 0 and smooth(W) and smooth(H) and uW % 2 == 0 and uH % 2 == 0 and smooth(uW) and smooth(uH) and uW <= 8192


def dct_forced():
    # input lengths 2 and 4 in both positions; the identity; every factor
    return [(2, 4, 2.0), (4, 2, 3.0), (2, 2, 1.0), (4, 4, 4.0), (48, 36, 1.0), (16, 24, 1.25), (20, 12, 1.5), (28, 50, 2.0), (24, 8, 2.5), (10, 14, 3.0),
            (6, 18, 4.0), (8, 192, 2.0)]


def dct_cases(n=None, s=None):
    def draw(rng):
        W, H = int(rng.choice(DCT_SMOOTH)), int(rng.choice(DCT_SMOOTH))
        u = float(rng.choice([1.0, 1.25, 1.5, 2.0, 2.0, 2.0, 2.5, 3.0, 4.0]))
        return (W, H, u) if dct_valid(W, H, u) and max(out_size(W, u), out_size(H, u)) <= 400 else None
    return _fill(dct_forced(), "dct", draw, n, s)


# ------------------------------------------------------------------------------------------------------------------- arm `view`
def view_valid(W, H, uW, uH, origin, span, any_flag):
    if min(W, H, uW, uH) < 2 or W > 8192:
        return False
    for s, M in ((span[0], uW), (span[1], uH)):
        if not (1.0 / 64 <= float(s) / M <= 8.0):
            return False
    if 2 * (W // 2) + uW > 8192 or conv_length(W, uW) > 8192 or 2 * (H // 2) + uH > 16384:
        return False
    if not (smooth(W) and smooth(H)) and not (any_flag and _bz_ok(W, H)):
        return False
    return view_col_tk(H, uH) != 0


def view_forced():
    in_ = 1.0 - 2.0 ** -30
    up = 1.0 + 2.0 ** -30
    out = []
    # the step span / M exactly 8 and exactly 1/64 on both axes, and just inside
    out += [(40, 36, 20, 18, (0.3, 0.7), (160.0, 144.0), 0), (40, 36, 20, 18, (0.3, 0.7), (160.0 * in_, 144.0 * in_), 0),
            (12, 10, 64, 128, (1.5, 2.5), (1.0, 2.0), 0), (12, 10, 64, 128, (1.5, 2.5), (1.0 * up, 2.0 * up), 0)]
    # step exactly 1: kmax = N/2 for an even N (the Nyquist bin with weight 1/2), (N - 1)/2 for an odd one; a step just above 1: one bin less
    out += [(30, 24, 20, 16, (3.0, 2.5), (20.0, 16.0), 0), (45, 21, 36, 15, (4.25, 1.5), (36.0, 15.0), 0),
            (30, 24, 20, 16, (3.0, 2.5), (20.0 * (1 + 2.0 ** -20), 16.0 * (1 + 2.0 ** -20)), 0)]
    # origins left of the frame and beyond it (the frame is periodic)
    out += [(48, 40, 40, 36, (-100.3, -7.75), (17.9, 12.2), 0), (48, 40, 40, 36, (1000.6, 95.25), (30.0, 50.5), 0)]
    # a non-smooth width, a non-smooth height, both; prime output lengths
    out += [(46, 24, 40, 30, (0.4, 0.6), (23.0, 11.0), 1), (24, 46, 30, 40, (0.5, -2.0), (30.0, 50.0), 1), (38, 58, 37, 41, (-1.0, 3.5), (40.0, 29.0), 1),
            (32, 20, 31, 43, (2.0, 1.0), (16.0, 20.0), 0)]
    # full frames (origin = the alignment's shift, span = the frame): the exact-size plans' map, which the exact-size oracle states too
    out += [(40, 30, 25, 48, ((40 / 25 - 1) / 2, (30 / 48 - 1) / 2), (40.0, 30.0), 0), (50, 32, 32, 50, (0.0, 0.0), (50.0, 32.0), 0)]
    # N = 2 under a large M, M = 2 over a large N
    out += [(2, 2, 64, 48, (0.25, -0.5), (2.0, 3.0), 0), (64, 48, 2, 2, (5.0, 7.0), (16.0, 9.0), 0)]
    # thin tall frames under the view rule: tile widths 4, 2 and 1; 4093 -> 4096: a Bluestein forward column and a convolution of 8192
    out += [(16, 600, 16, 700, (0.5, 10.25), (16.0, 580.0), 0), (16, 1200, 16, 1300, (0.0, -3.5), (16.0, 1200.0), 0),
            (16, 2400, 16, 2600, (1.5, 0.75), (12.0, 2400.0), 0), (8, 4093, 8, 4096, (0.0, 100.5), (8.0, 6.0 * 4096), 1)]
    return out


def view_cases(n=None, s=None):
    def draw(rng):
        W, H, uW, uH = (int(x) for x in rng.integers(2, 201, 4))
        if rng.random() < 0.5:                                                     # (half of them without a Bluestein transform)
            W, H = int(rng.choice(SMOOTH_ANY)), int(rng.choice(SMOOTH_ANY))
        step = 2.0 ** rng.uniform(-4.0, 2.5, 2)
        span = (float(uW * step[0]), float(uH * step[1]))
        origin = (float(rng.uniform(-1.5, 1.5) * W), float(rng.uniform(-1.5, 1.5) * H))
        any_flag = int(not (smooth(W) and smooth(H)))
        c = (W, H, uW, uH, origin, span, any_flag)
        return c if view_valid(*c) else None
    return _fill(view_forced(), "view", draw, n, s)


CASES = {"exact": exact_cases, "odd": odd_cases, "any": any_cases, "down": down_cases, "dct": dct_cases, "view": view_cases}


def precision_and_input(arm, n, s=None):
    """(precision, uint8 input) of the arm's n cases: the four pairs dealt in shuffled blocks of four, so that every pair runs on a
    quarter of the cases (rounded down)"""
    rng = np.random.default_rng((seed() if s is None else s) + OFFSET[arm] + 7)
    out = []
    while len(out) < n:
        out += [((0, 2)[k // 2], bool(k % 2)) for k in rng.permutation(4)]
    return out[:n]
