"""Strengths and tone regimes for the sharpen kernels, and the bars their tests use.  Test infrastructure only: no test lives here and
nothing needs a device (tests/test_host_sharpen_regimes.py proves the table and the bars on the CPU, tests/test_gpu_sharpen_regimes.py
holds every sharpen kernel to them).

The filter (oracle/fftup_oracle.c, sharpen_plane): len = min(|upsq R|, 1) per tap, mn / mx the means of the cross and the 3x3 minima /
maxima, a = mn / (1 - mn), b = (1 - mx) / mx, scale = -s sqrt(min(a, b)), out = (C + scale s4) / (1 + 4 scale).  a < b <=> mn + mx < 1:
dark neighbourhoods take the minimum's quotient, bright ones the maximum's; den = 1 + 4 scale reaches 0 for s >= 0.25 (a pole of the
filter: the cases the issue names POLES, which no table row may be).

Frames: planes() = tone + amp * tex, tex periodic (two cosines with whole numbers of cycles per frame) plus a little noise, as planar
floats -- values outside [0, 1] are legal there.  REGIMES names the (tone, amp) pairs, STRENGTHS the strengths; CASES is the literal
table, one row per (regime, strength) with the comparisons it is fit for:
    iso   the kernel alone, fp32 / fp64: its output against oraclelib.sharpen of the DEVICE's own pre-sharpen planes
    e2e   fp32 end to end (and fused against unfused): against the oracle's output
    p2    binary16, end to end or fused
A mark is a claim about the ORACLE alone: the bar below, computed from the oracle's own pre-sharpen image, is under the ceiling of
its kind (ISO_CEILING, E2E_CEILING, P2_CEILING: the project's loosest existing bars for uniform noise), and the oracle's output is
finite.  conditions() evaluates exactly that; the CPU test holds every row to it at the shapes of the stand-alone sharpen kernels.

Bars.  None is fitted to a kernel: each is the oracle's own response to a perturbation of its input R that the project already
allows, probe(R, move) = max over K seeded random-sign patterns of max |sharpen(move(R, sign)) - sharpen(R)|.
    T_iso = 16 probe(R (1 + eps sign)) + 4 eps, eps = 2^-23 (fp32) or 2^-52 (fp64).  Backward error: an evaluator chain of at most
        12 rounded operations (scaling by upsq, the two sums of minima / maxima, 1 - x, the product or quotient n d, root, the product
        with the strength, s4's three additions, the two fused multiply-adds or their four operations) plus two hardware seeds of one
        ulp each (rsq, rcp), 14 relative errors of eps in all, rounded up to a power of two; the output's own rounding and that of a
        result near 1 are the 4 eps.  The count changes only with that argument.
    T_e2e = max(FP32_OUT_MAX, 2 probe(R + (FP32_PRE_MAX / sc) sign)): FP32_PRE_MAX / sc is the transform error the project already
        allows on R (paritylib); the 2 covers the gap between random sign patterns and the worst one.
    T16 = 2 probe(every value moved one binary16 ulp, random direction), in the oracle's binary16 arithmetic; and the share of
        differing outputs at most f_ref + NATIVE_RCP_FRAC, f_ref the share of oracle outputs that change when FP16_PRE_DIFF_FRAC of
        the inputs move one ulp, NATIVE_RCP_FRAC = 5e-3 the allowance test_fused_sharpen_equals_unfused already gives the
        native-reciprocal evaluator.
    -p 1 end to end (the non-R2C path, where no isolation exists): T_e2e with FP64_PRE_MAX = 1e-12 and the floor FP64_OUT_MAX = 1e-9,
        the bars of tests/test_gpu_parity.py::test_fp64_parity.
    The non-R2C path sharpens a complex image (taps |u^2 z|): there the probes move both parts of z, each with signs of its own, and
        run the oracle's filter of the complex image (oraclelib.sharpen_complex).
"""
import numpy as np

import oraclelib as O
from paritylib import FP16_PRE_DIFF_FRAC, FP32_OUT_MAX, FP32_PRE_MAX, measured

# ---------------------------------------------------------------------------------------------------------------------- the cases
REGIMES = {
    "black_flat": (0.0, 0.0),
    "black_signs": (0.0, 0.02),          # sign changes around black
    "near_black": (0.02, 0.02),
    "dark": (0.1, 0.05),
    "low": (0.25, 0.1),
    "mid_flat": (0.5, 0.0),              # the tie mn + mx == 1
    "mid_fine": (0.5, 0.02),
    "mid_wide": (0.5, 0.2),
    "high": (0.75, 0.1),
    "bright": (0.95, 0.04),
    "white_flat": (1.0, 0.0),
    "white_half_clamped": (1.0, 0.03),
    "all_clamped": (1.3, 0.2),
    "negative": (-0.3, 0.1),
    "zero_crossing": (0.0, 0.3),
}
STRENGTHS = (0.0, 0.05, 0.24, 0.5, 1.0, -0.2, 0.1234567, 4e-7)       # (0.2 stays with the existing tests; "%f" of the last two:
#                                                                       0.123457 and 0.000000)
# den = 1 + 4 scale crosses 0 inside the frame: amplification 1e3 .. 1e9, the binary16 oracle returns inf.  Never a table row.
POLES = (("dark", 1.0), ("low", 0.5), ("high", 0.5), ("bright", 1.0), ("negative", 0.5), ("zero_crossing", 0.5), ("zero_crossing", 1.0))

ISO_CEILING = 1e-4       # tests/test_gpu_parity.py: the sharpen kernel alone on uniform noise
E2E_CEILING = 5e-4       # ... end to end on uniform noise (and tests/test_gpu_sweep.py)
P2_CEILING = 1.6e-2      # tests/test_gpu_sweep.py, -p 2
NATIVE_RCP_FRAC = 5e-3   # tests/test_gpu_parity.py::test_fused_sharpen_equals_unfused, -p 2
FP64_PRE_MAX = 1e-12     # tests/test_gpu_parity.py::test_fp64_parity
FP64_OUT_MAX = 1e-9
EPS = {0: 2.0 ** -23, 1: 2.0 ** -52}
CPLX_P1_W = 2058         # the smallest -p 1 width on the non-R2C path at -u 2: uW = 4116 > 4096, 2058 = 2 3 7^3
JIT_SMALLEST = {2.0: (64, 64), 1.5: (64, 64)}      # the smallest sizes (by area) with kernels specialised at plan time
K_PROBES = 3

# (regime, strength, marks): literal.  Derived with the oracle's own pipeline (upscale_planes of planes()) at the shapes of the
# stand-alone kernels, 28x12 -u 1.5 and 256x24 -u 2: a mark stands where conditions() holds at both.
CASES = (
    ("black_flat", 0.0, "iso e2e p2"),
    ("black_flat", 0.05, "iso e2e p2"),
    ("black_flat", 0.24, "iso e2e p2"),
    ("black_flat", 0.5, "iso e2e p2"),
    ("black_flat", 1.0, "iso e2e p2"),
    ("black_flat", -0.2, "iso e2e p2"),
    ("black_flat", 0.1234567, "iso e2e p2"),
    ("black_flat", 4e-07, "iso e2e p2"),
    ("black_signs", 0.0, "iso e2e p2"),
    ("black_signs", 0.05, "iso e2e p2"),
    ("black_signs", 0.24, "iso e2e p2"),
    ("black_signs", 0.5, "iso e2e p2"),
    ("black_signs", 1.0, "iso e2e p2"),
    ("black_signs", -0.2, "iso e2e p2"),
    ("black_signs", 0.1234567, "iso e2e p2"),
    ("black_signs", 4e-07, "iso e2e p2"),
    ("near_black", 0.0, "iso e2e p2"),
    ("near_black", 0.05, "iso e2e p2"),
    ("near_black", 0.24, "iso e2e p2"),
    ("near_black", 0.5, "iso e2e p2"),
    ("near_black", 1.0, "iso e2e p2"),
    ("near_black", -0.2, "iso e2e p2"),
    ("near_black", 0.1234567, "iso e2e p2"),
    ("near_black", 4e-07, "iso e2e p2"),
    ("dark", 0.0, "iso e2e p2"),
    ("dark", 0.05, "iso e2e p2"),
    ("dark", 0.24, "iso e2e p2"),
    ("dark", 0.5, "iso e2e p2"),
    ("dark", -0.2, "iso e2e p2"),
    ("dark", 0.1234567, "iso e2e p2"),
    ("dark", 4e-07, "iso e2e p2"),
    ("low", 0.0, "iso e2e p2"),
    ("low", 0.05, "iso e2e p2"),
    ("low", 0.24, "iso e2e p2"),
    ("low", 1.0, "iso e2e p2"),
    ("low", -0.2, "iso e2e p2"),
    ("low", 0.1234567, "iso e2e p2"),
    ("low", 4e-07, "iso e2e p2"),
    ("mid_flat", 0.0, "iso e2e p2"),
    ("mid_flat", 0.05, "iso e2e p2"),
    ("mid_flat", 0.24, "iso"),
    ("mid_flat", 0.5, "iso e2e p2"),
    ("mid_flat", 1.0, "iso e2e p2"),
    ("mid_flat", -0.2, "iso e2e p2"),
    ("mid_flat", 0.1234567, "iso e2e p2"),
    ("mid_flat", 4e-07, "iso e2e p2"),
    ("mid_fine", 0.0, "iso e2e p2"),
    ("mid_fine", 0.05, "iso e2e p2"),
    ("mid_fine", 0.24, "iso"),
    ("mid_fine", 0.5, "iso e2e p2"),
    ("mid_fine", 1.0, "iso e2e p2"),
    ("mid_fine", -0.2, "iso e2e p2"),
    ("mid_fine", 0.1234567, "iso e2e p2"),
    ("mid_fine", 4e-07, "iso e2e p2"),
    ("mid_wide", 0.0, "iso e2e p2"),
    ("mid_wide", 0.05, "iso e2e p2"),
    ("mid_wide", 0.24, "iso"),
    ("mid_wide", 0.5, "iso e2e p2"),
    ("mid_wide", 1.0, "iso e2e p2"),
    ("mid_wide", -0.2, "iso e2e p2"),
    ("mid_wide", 0.1234567, "iso e2e p2"),
    ("mid_wide", 4e-07, "iso e2e p2"),
    ("high", 0.0, "iso e2e p2"),
    ("high", 0.05, "iso e2e p2"),
    ("high", 0.24, "iso e2e p2"),
    ("high", 1.0, "iso e2e p2"),
    ("high", -0.2, "iso e2e p2"),
    ("high", 0.1234567, "iso e2e p2"),
    ("high", 4e-07, "iso e2e p2"),
    ("bright", 0.0, "iso e2e p2"),
    ("bright", 0.05, "iso e2e p2"),
    ("bright", 0.24, "iso e2e p2"),
    ("bright", 0.5, "iso e2e p2"),
    ("bright", -0.2, "iso e2e p2"),
    ("bright", 0.1234567, "iso e2e p2"),
    ("bright", 4e-07, "iso e2e p2"),
    ("white_flat", 0.0, "iso e2e p2"),
    ("white_flat", 0.05, "iso e2e p2"),
    ("white_flat", 0.24, "iso e2e p2"),
    ("white_flat", 0.5, "iso e2e p2"),
    ("white_flat", 1.0, "iso e2e p2"),
    ("white_flat", -0.2, "iso e2e p2"),
    ("white_flat", 0.1234567, "iso e2e p2"),
    ("white_flat", 4e-07, "iso e2e p2"),
    ("white_half_clamped", 0.0, "iso e2e p2"),
    ("white_half_clamped", 0.05, "iso e2e p2"),
    ("white_half_clamped", 0.24, "iso e2e p2"),
    ("white_half_clamped", 0.5, "iso e2e p2"),
    ("white_half_clamped", 1.0, "iso e2e p2"),
    ("white_half_clamped", -0.2, "iso e2e p2"),
    ("white_half_clamped", 0.1234567, "iso e2e p2"),
    ("white_half_clamped", 4e-07, "iso e2e p2"),
    ("all_clamped", 0.0, "iso e2e p2"),
    ("all_clamped", 0.05, "iso e2e p2"),
    ("all_clamped", 0.24, "iso e2e p2"),
    ("all_clamped", 0.5, "iso e2e p2"),
    ("all_clamped", 1.0, "iso e2e p2"),
    ("all_clamped", -0.2, "iso e2e p2"),
    ("all_clamped", 0.1234567, "iso e2e p2"),
    ("all_clamped", 4e-07, "iso e2e p2"),
    ("negative", 0.0, "iso e2e p2"),
    ("negative", 0.05, "iso e2e p2"),
    ("negative", 0.24, "iso e2e p2"),
    ("negative", 1.0, "iso e2e p2"),
    ("negative", -0.2, "iso e2e p2"),
    ("negative", 0.1234567, "iso e2e p2"),
    ("negative", 4e-07, "iso e2e p2"),
    ("zero_crossing", 0.0, "iso e2e p2"),
    ("zero_crossing", 0.05, "iso e2e p2"),
    ("zero_crossing", 0.24, "iso e2e p2"),
    ("zero_crossing", -0.2, "iso e2e p2"),
    ("zero_crossing", 0.1234567, "iso e2e p2"),
    ("zero_crossing", 4e-07, "iso e2e p2"),
)


def rows(mark):
    return [(r, s) for (r, s, marks) in CASES if mark in marks.split()]


def case_id(regime, s):
    return "%s-s%.7g" % (regime, s)


# --------------------------------------------------------------------------------------------------------------------- the frames
def _dtype(precision):
    return {0: np.float32, 1: np.float64, 2: np.float16}[precision]


def tex(W, H, seed):
    """[3][H][W], max |tex| = 1 per channel: two cosines with whole numbers of cycles per frame (periodic: no border ringing), each
    channel shifted differently, plus 0.15 sigma Gaussian noise"""
    rng = np.random.RandomState(1000 + seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((3, H, W))
    for c in range(3):
        px, py = rng.rand(2) * 2.0 * np.pi
        t = np.cos(2.0 * np.pi * (3.0 * x / W + 1.0 * y / H) + px) + 0.6 * np.cos(2.0 * np.pi * (7.0 * x / W - 2.0 * y / H) + py)
        t += 0.15 * rng.randn(H, W)
        out[c] = t / np.abs(t).max()
    return out


def planes(W, H, tone, amp, seed, precision=0):
    """[3][H][W] = tone + amp * tex in the plan's storage type (upload_planar takes it as it is)"""
    return (tone + amp * tex(W, H, seed)).astype(_dtype(precision))


def regime_planes(W, H, regime, precision=0):
    tone, amp = REGIMES[regime]
    return planes(W, H, tone, amp, sorted(REGIMES).index(regime), precision)


def regime_codes(W, H, regime):
    """the frame as 8-bit codes [H][W][3] (upload_rgb8), for the regimes inside [0, 1]"""
    p = regime_planes(W, H, regime, 1)
    assert p.min() >= 0.0 and p.max() <= 1.0
    return np.ascontiguousarray(np.transpose(np.rint(255.0 * p), (1, 2, 0)).astype(np.uint8))


def const_text(v, precision):
    """a constant as the filter sees it: the float through "%f" text (six decimals), parsed in the arithmetic's type"""
    t = float("%f" % float(np.float32(v)))
    return float(np.float16(t)) if precision == 2 else float(np.float32(t))


# ----------------------------------------------------------------------------------------------------------------------- the bars
def _signs(shape, seed, k, cplx=False):
    sg = np.random.RandomState(77 + 131 * seed + k).randint(0, 2, shape) * 2.0 - 1.0
    return sg + 1j * _signs(shape, seed + 7, k) if cplx else sg


def _filter(R):
    """the oracle's filter for a real image, or for the complex image of the non-R2C path (taps |u^2 z|)"""
    return O.sharpen_complex if np.iscomplexobj(R) else O.sharpen


def probe(R, u, precision, s, move, K=K_PROBES, seed=0, base=None):
    """max over K seeded sign patterns of max |sharpen(move(R, sign)) - sharpen(R)| (inf where the oracle's output is not finite).
    A complex R (the non-R2C path) is moved in both parts, each with signs of its own."""
    f = _filter(R)
    base = f(R, u, precision, s) if base is None else base
    worst = 0.0
    for k in range(K):
        with np.errstate(invalid="ignore"):              # (inf - inf at a pole)
            d = np.abs(f(move(R, _signs(R.shape, seed, k, np.iscomplexobj(R))), u, precision, s) - base)
        worst = max(worst, float(d.max()) if np.isfinite(d).all() else np.inf)
    return worst if np.isfinite(base).all() else np.inf


def half_step(R16, sign):
    """every binary16 value of R16 (as float64) moved one ulp in the direction of `sign`; 0 keeps a value (complex: per part)"""
    if np.iscomplexobj(R16):
        return half_step(R16.real, np.real(sign)) + 1j * half_step(R16.imag, np.imag(sign))
    h = R16.astype(np.float16)
    up = np.nextafter(h, np.float16(np.inf))
    dn = np.nextafter(h, np.float16(-np.inf))
    return np.where(sign > 0, up, np.where(sign < 0, dn, h)).astype(np.float64)


def t_iso(R, u, precision, s, K=K_PROBES, base=None):
    eps = EPS[precision]
    return 16.0 * probe(R, u, precision, s, lambda r, sg: r * (1.0 + eps * sg), K, base=base) + 4.0 * eps


def t_e2e(R, u, precision, s, K=K_PROBES, base=None):
    """precision 0 or 1; sc = u * u, the factor between the stored R and the amplitude-preserving image"""
    pre_max, floor = (FP32_PRE_MAX, FP32_OUT_MAX) if precision == 0 else (FP64_PRE_MAX, FP64_OUT_MAX)
    step = pre_max / (float(np.float32(u)) ** 2)
    return max(floor, 2.0 * probe(R, u, precision, s, lambda r, sg: r + step * sg, K, base=base))


def t16(R16, u, s, K=K_PROBES, base=None):
    return 2.0 * probe(R16, u, 2, s, half_step, K, base=base)


def f_ref(R16, u, s, base=None):
    """the share of the binary16 oracle's outputs that change when FP16_PRE_DIFF_FRAC of its inputs move one ulp"""
    f = _filter(R16)
    base = f(R16, u, 2, s) if base is None else base
    rng = np.random.RandomState(4242)

    def some(shape):
        return np.where(rng.rand(*shape) < FP16_PRE_DIFF_FRAC, rng.randint(0, 2, shape) * 2.0 - 1.0, 0.0)
    sg = some(R16.shape) + 1j * some(R16.shape) if np.iscomplexobj(R16) else some(R16.shape)
    return float((f(half_step(R16, sg), u, 2, s) != base).mean())


def oracle_R(x, u, precision, s):
    """(the oracle's pre-sharpen image, its output) for the input planes x: the real pipeline"""
    pre, out, _ = O.upscale_planes(np.asarray(x, np.float64), u, precision, s)
    return pre, out


def conditions(W, H, u, regime, s, K=K_PROBES):
    """{mark: (bar, holds)} from the oracle alone: holds = the bar is finite and under the ceiling of its kind"""
    res = {}
    R, out = oracle_R(regime_planes(W, H, regime, 0), u, 0, s)
    fin = bool(np.isfinite(out).all())
    ti, te = t_iso(R, u, 0, s, K, base=out), t_e2e(R, u, 0, s, K, base=out)
    res["iso"] = (ti, fin and ti <= ISO_CEILING)
    res["e2e"] = (te, fin and te <= E2E_CEILING)
    R16, out16 = oracle_R(regime_planes(W, H, regime, 2), u, 2, s)
    th = t16(R16, u, s, K, base=out16)
    res["p2"] = (th, bool(np.isfinite(out16).all()) and th <= P2_CEILING)
    return res


# ---------------------------------------------------------------------------------------------------------------- the comparisons
def assert_iso(tag, out, R_dev, u, precision, s, K=K_PROBES):
    """the kernel alone: `out` against the oracle's filter of the planes the kernel read, at T_iso of those planes"""
    want = O.sharpen(R_dev, u, precision, s)
    bar = t_iso(R_dev, u, precision, s, K, base=want)
    err = float(np.abs(np.asarray(out, np.float64) - want).max())
    measured(tag, iso_max=err, T_iso=bar)
    assert np.isfinite(want).all() and np.isfinite(out).all()
    assert bar <= ISO_CEILING
    assert err <= bar
    return err, bar


def assert_e2e(tag, out, want, R, u, precision, s, K=K_PROBES, bar=None):
    """fp32 / fp64 end to end, or fused against unfused: `out` against `want` at T_e2e of the pre-sharpen image R"""
    bar = t_e2e(R, u, precision, s, K) if bar is None else bar
    err = float(np.abs(np.asarray(out, np.float64) - want).max())
    measured(tag, e2e_max=err, T_e2e=bar)
    assert np.isfinite(want).all() and np.isfinite(out).all()
    assert bar <= E2E_CEILING
    assert err <= bar
    return err, bar


def assert_p2(tag, out, want, R16, u, s, K=K_PROBES, bars=None):
    """binary16 end to end or fused: max |out - want| within T16 of R16, and differing in at most f_ref + NATIVE_RCP_FRAC of the values"""
    bar, fr = (t16(R16, u, s, K), f_ref(R16, u, s)) if bars is None else bars
    out = np.asarray(out, np.float64)
    err, frac = float(np.abs(out - want).max()), float((out != want).mean())
    measured(tag, p2_max=err, T16=bar, diff_frac=frac, frac_bar=fr + NATIVE_RCP_FRAC)
    assert np.isfinite(want).all() and np.isfinite(out).all()
    assert bar <= P2_CEILING
    assert err <= bar
    assert frac <= fr + NATIVE_RCP_FRAC
    return err, bar
