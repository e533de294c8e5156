"""GPU: seeded sweeps over the plan families added after tests/test_gpu_sweep.py -- exact-size, odd-size, any-size, downscale (FFT
and DCT), DCT upscale and view plans -- each case against its family's own oracle through its family's own _check, at the
project's bars exactly as tests/paritylib.py states them.  No bar is stated or widened here.

The cases come from tests/family_sweep_cases.py: per arm a forced part (the strata: lengths of 2 and 3, every parity class of an
axis at both alignments, folded and split Nyquist bins, Bluestein lengths of 2N - 1, column tile widths 4, 2 and 1, a column pass
just under the LDS limit, every residue of the spectrum's column count modulo the tile width, views at the bounds of the step ...)
and a random fill up to FFTUP_FAMILY_SWEEP_N cases (FFTUP_BIG_TESTS=1: a larger default), seeded by FFTUP_SWEEP_SEED.
tests/test_host_family_sweep.py shows on the CPU that the planner accepts every case -- there is no skip path here -- and that the
strata are reached under three seeds.

Precision (-p 0, -p 2) and input kind (planar, fused uint8) are dealt per case, a quarter of an arm's cases to each pair.  The
-p 2 bars on the FRACTION of differing values (<= 1 % of R, <= 2 % of the output) mean nothing on an output of a few dozen values:
a case whose output has fewer values than the smallest case of its family's existing -p 2 parity list (TINY below, read off those
lists) runs -p 0 in the parametrized test and -p 2 in one pooled test per arm, which asserts the one-ulp bound, the output's L2 and
max bars per case and the two fraction bars on the pooled counts.  M = N / -u 1 cases also meet the identity bar of the family
modules (paritylib.assert_identity).

Worst values measured on an MI355X, default run / one-off run of 100 cases per arm (profiles/family_sweep_long.txt; default seed).
-p 0 (bars: paritylib.FP32_*, in the columns' order; the identity's are the first two):
    arm    pre_l2            pre_max           out_l2            out_max           identity l2, max (the larger run)
    exact  2.9e-7 / 2.9e-7   7.1e-7 / 8.9e-7   7.2e-7 / 7.3e-7   2.1e-6 / 2.4e-6   2.7e-7, 6.6e-7
    odd    2.7e-7 / 3.3e-7   6.0e-7 / 7.9e-7   6.8e-7 / 7.6e-7   1.8e-6 / 2.4e-6   (no -u 1 among the factors)
    any    2.9e-7 / 3.4e-7   7.0e-7 / 8.3e-7   5.9e-7 / 7.1e-7   2.0e-6 / 2.3e-6   3.1e-7, 6.6e-7
    down   1.6e-7 / 1.8e-7   3.2e-7 / 3.4e-7   3.9e-7 / 3.9e-7   1.0e-6 / 1.1e-6
    dct    1.6e-7 / 1.8e-7   3.8e-7 / 4.2e-7   3.5e-7 / 3.8e-7   1.1e-6 / 1.2e-6   1.8e-7, 3.3e-7
    view   3.1e-7 / 3.5e-7   6.5e-7 / 8.5e-7   6.8e-7 / 7.7e-7   1.8e-6 / 2.7e-6
-p 2, parametrized cases (bars: paritylib.FP16_* and the one-ulp bound, in the columns' order):
    arm    differing R          ulps of R     out_l2            out_max           differing output
    exact  0.87 % / 0.87 %      0.99 / 0.99   2.2e-4 / 2.2e-4   2.4e-3 / 2.4e-3   1.98 % / 1.98 %
    odd    0.040 % / 0.051 %    0.99 / 1.0    5.0e-5 / 5.5e-5   2.4e-3 / 2.4e-3   0.084 % / 0.11 %
    any    0.041 % / 0.043 %    1.0 / 1.0     6.1e-5 / 6.4e-5   2.9e-3 / 2.9e-3   0.076 % / 0.086 %
    down   0.025 % / 0.046 %    0.64 / 0.91   4.7e-5 / 4.7e-5   1.5e-3 / 1.9e-3   0.067 % / 0.12 %
    dct    0.0093 % / 0.023 %   0.95 / 1.0    2.7e-5 / 5.1e-5   1.9e-3 / 2.2e-3   0.014 % / 0.059 %
    view   0.098 % / 0.098 %    0.99 / 1.0    1.3e-4 / 1.3e-4   2.4e-3 / 2.9e-3   0.23 % / 0.23 %
-p 2, tiny outputs: per case ulps of R <= 1.0, out_l2 <= 1.1e-4, out_max <= 2.4e-3 in every arm and both runs; the pooled fractions
of R and of the output stay at or below 0.029 % and 0.057 % (odd, default run).
The headroom is a factor of about ten on the -p 0 bars and on the fractions, three on the -p 2 maxima, with one exception: 48x30 ->
48x48 (a forced case, planar binary16 input).  Its rows are M = N and every eighth output row sits on an input row, where R = 5/8 x
in exact arithmetic: 168 of the 6912 values are exact ties between two binary16 numbers, which the fp64 oracle and the fp32 kernels
break by their own last bits; the other 99 % of that case differ as rarely as everywhere else.
The DCT downscale cases at factors whose upsq = "%f"(u u) is no binary16 number (0.4, 0.8, 2/3 ...) failed the first run at -p 2:
tests/test_gpu_downscale.py divided by the fp32 constant where the plan divides by the binary16 one -- fixed there.
Wall time of the default run (234 tests), same machine and session: 9.5 s, beside 17.8 s of tests/test_gpu_sweep.py and 5.6 s of
tests/test_gpu_exactsize.py; FFTUP_BIG_TESTS=1: 470 tests, 19 s.
"""
import numpy as np
import pytest

import downscale_oracle as S
import family_sweep_cases as F
import oddsize_oracle as Q
import oraclelib as O
import paritylib as P
import test_gpu_anysize as A
import test_gpu_dct as DC
import test_gpu_downscale as DN
import test_gpu_exactsize as EX
import test_gpu_oddsize as OD
import test_gpu_view as VW

pytestmark = pytest.mark.gpu

# values (3 planes) of the smallest output among the family's cases that run -p 2 today
TINY = {
    "exact": min(3 * uW * uH for _, _, uW, uH, _ in EX.SMALL),
    "odd": min(3 * Q.out_size(W, u) * Q.out_size(H, u) for W, H, u, _, p, _ in OD.CASES if p == 2),
    "any": min([3 * Q.out_size(W, u) * Q.out_size(H, u) for W, H, u in A.UP] + [3 * S.out_size(W, u) * S.out_size(H, u) for W, H, u, p in A.DOWN if p == 2]),
    "down": min(3 * S.out_size(W, u) * S.out_size(H, u) for W, H, u in DN.SIZES + DN.SIZES_DCT),
    "dct": min(3 * Q.out_size(W, u) * Q.out_size(H, u) for W, H, u in DC.SIZES_FP16),
    "view": min(3 * c[2] * c[3] for c in VW.VIEWS + VW.THIN),
}


def _out_values(arm, c):
    if arm in ("exact", "view"):
        return 3 * c[2] * c[3]
    return 3 * F.out_size(c[0], c[2]) * F.out_size(c[1], c[2])


def _rows(arm):
    """(index, case, precision, uint8) of the arm's list"""
    cases = F.CASES[arm]()
    return [(k, c, p, u8) for k, (c, (p, u8)) in enumerate(zip(cases, F.precision_and_input(arm, len(cases))))]


def _params(arm):
    """every case once: a tiny case at -p 0 (its -p 2 run is the pooled test's)"""
    return [pytest.param(k, c, 0 if _out_values(arm, c) < TINY[arm] else p, u8, id="%d-%s" % (k, "x".join(str(x) for x in c[:4] if not isinstance(x, (str, bool, tuple)))))
            for k, c, p, u8 in _rows(arm)]


def _tiny(arm):
    return [(k, c, u8) for k, c, _, u8 in _rows(arm) if _out_values(arm, c) < TINY[arm]]


def _identity(tag, pre, x):
    P.assert_identity(tag + " identity", pre, x)


def _case(arm, k, c, p, u8, pooled=None):
    tag = "sweep %s %d p%d %s u8%d" % (arm, k, p, " ".join(str(x) for x in c), u8)
    seed = 5000 + k
    if arm == "exact":
        W, H, uW, uH, align, any_flag = c
        pre, x = EX._check(W, H, uW, uH, p, "any" if any_flag else "", align, u8, seed, tag, pooled=pooled)
        if (W, H) == (uW, uH) and p == 0:
            _identity(tag, pre, x)
    elif arm == "odd":
        W, H, u, extra = c
        pre, x = OD._check(W, H, u, p, extra, u8, seed, tag, pooled=pooled)
        if u == 1.0 and p == 0:
            _identity(tag, pre, x)
    elif arm == "any":
        W, H, u, down = c
        pre, x = A._check(W, H, u, p, down, u8, seed, tag, pooled=pooled)
        if u == 1.0 and p == 0:
            _identity(tag, pre, x)
    elif arm == "down":
        W, H, u, dct = c
        DN._check(W, H, u, p, dct, u8, seed, tag, pooled=pooled)
    elif arm == "dct":
        W, H, u = c
        pre, rgb = DC._check(W, H, u, p, u8, seed, tag, pooled=pooled)
        if u == 1.0 and p == 0:
            _identity(tag, pre, O.load_lut(0)[np.transpose(rgb, (2, 0, 1))])
    else:
        W, H, uW, uH, origin, span, any_flag = c
        VW._check(W, H, uW, uH, origin, span, p, "any" if any_flag else "", u8, seed, tag, pooled=pooled)


def _pooled(arm):
    """the arm's tiny cases at -p 2: the per-case bars inside _check, the two fraction bars on all of them together"""
    acc = []
    for k, c, u8 in _tiny(arm):
        _case(arm, k, c, 2, u8, pooled=acc)
    if acc:
        P.pooled_fraction_bars("sweep %s pooled p2 (%d cases)" % (arm, len(acc)), acc)


@pytest.mark.parametrize("k,c,p,u8", _params("exact"))
def test_exact_sweep(k, c, p, u8):
    _case("exact", k, c, p, u8)


def test_exact_sweep_tiny_outputs_p2():
    _pooled("exact")


@pytest.mark.parametrize("k,c,p,u8", _params("odd"))
def test_odd_sweep(k, c, p, u8):
    _case("odd", k, c, p, u8)


def test_odd_sweep_tiny_outputs_p2():
    _pooled("odd")


@pytest.mark.parametrize("k,c,p,u8", _params("any"))
def test_any_sweep(k, c, p, u8):
    _case("any", k, c, p, u8)


def test_any_sweep_tiny_outputs_p2():
    _pooled("any")


@pytest.mark.parametrize("k,c,p,u8", _params("down"))
def test_down_sweep(k, c, p, u8):
    _case("down", k, c, p, u8)


def test_down_sweep_tiny_outputs_p2():
    _pooled("down")


@pytest.mark.parametrize("k,c,p,u8", _params("dct"))
def test_dct_sweep(k, c, p, u8):
    _case("dct", k, c, p, u8)


def test_dct_sweep_tiny_outputs_p2():
    _pooled("dct")


@pytest.mark.parametrize("k,c,p,u8", _params("view"))
def test_view_sweep(k, c, p, u8):
    _case("view", k, c, p, u8)


def test_view_sweep_tiny_outputs_p2():
    _pooled("view")
