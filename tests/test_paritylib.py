"""CPU: the comparison code of tests/paritylib.py rejects what it should.  A synthetic 3x64x64 image stands in for a plan's
pre-sharpen image and output (oraclelib.sharpen is the only native code involved); every test builds an error on purpose, checks
with the paritylib primitives which bars that error violates, and then that assert_parity does or does not raise.

3x64x64: the norm of the image is about 64, so one value off by a little more than a max bar moves the relative L2 error by
max / 64 -- a twelfth and a sixteenth of the matching L2 bar at -p 0, four tenths of it at -p 2 -- and 1 % of the values is 123 of
them."""
import numpy as np
import pytest

import oraclelib as O
import paritylib as P

SC, U = 4.0, 2.0                    # R = y / 4 exactly
P0_BARS = ["pre_l2", "pre_max", "out_l2", "out_max"]
P2_BARS = ["pre_ulp", "pre_diff_frac", "out_l2", "out_max", "out_diff_frac"]


@pytest.fixture(scope="module")
def ref():
    """the oracle side, computed once and read-only: y, and per precision (what the plan stores, its sharpened image)"""
    R = np.random.RandomState(7).rand(3, 64, 64) * 0.9 + 0.05
    opre = R.astype(np.float16).astype(np.float64)
    d = {"y": SC * R, 0: (R, O.sharpen(R, U, 0, P.SHARPEN)), 2: (opre, O.sharpen(opre, U, 2, P.SHARPEN))}
    for a in (d["y"],) + d[0] + d[2]:
        a.setflags(write=False)
    return d


def _violated(precision, pre, out, ref):
    """the names of the bars the pair misses, by the paritylib primitives"""
    stored, sh = ref[precision]
    if precision == 0:
        holds = {"pre_l2": P.rel_l2(SC * pre, ref["y"]) <= P.FP32_PRE_L2, "pre_max": np.abs(SC * pre - ref["y"]).max() <= P.FP32_PRE_MAX,
                 "out_l2": P.rel_l2(out, sh) <= P.FP32_OUT_L2, "out_max": np.abs(out - sh).max() <= P.FP32_OUT_MAX}
    else:
        holds = {"pre_ulp": P.within_one_half_ulp(pre, stored).all(), "pre_diff_frac": (pre != stored).mean() <= P.FP16_PRE_DIFF_FRAC,
                 "out_l2": P.rel_l2(out, sh) <= P.FP16_OUT_L2, "out_max": np.abs(out - sh).max() <= P.FP16_OUT_MAX,
                 "out_diff_frac": (out != sh).mean() <= P.FP16_OUT_DIFF_FRAC}
    return sorted(k for k, ok in holds.items() if not ok)


def _some(a, frac, seed=1):
    """a boolean mask over `a` with round(frac * size) values set, none of them in the last row"""
    m = np.zeros(a.size, bool)
    inner = np.arange(a.size).reshape(a.shape)[:, :-1].ravel()
    m[np.random.RandomState(seed).choice(inner, int(round(frac * a.size)), replace=False)] = True
    return m.reshape(a.shape)


def _signs(a, seed=2):
    return np.random.RandomState(seed).choice([-1.0, 1.0], a.shape)


def _uniform(a, rel):
    """`a` plus an error of one magnitude everywhere, relative L2 error `rel`"""
    return a + _signs(a) * rel * np.linalg.norm(a) / np.sqrt(a.size)


def _one_step(a, mask):
    """`a` (binary16 values) with the masked values moved to their upper binary16 neighbour"""
    up = np.nextafter(a.astype(np.float16), np.float16(np.inf)).astype(np.float64)
    return np.where(mask, up, a)


def _pair(precision, bar, ref):
    """(pre, out) built to miss `bar` and no other bar; bar None: just inside every bar"""
    stored, sh = ref[precision]
    pre, out = stored.copy(), sh.copy()
    if precision == 0:
        if bar is None:
            pre = _uniform(stored, 0.9 * P.FP32_PRE_L2)
            pre[1, 3, 5] = stored[1, 3, 5] + 0.95 * P.FP32_PRE_MAX / SC
            out = _uniform(sh, 0.9 * P.FP32_OUT_L2)
            out[2, 7, 9] = sh[2, 7, 9] - 0.95 * P.FP32_OUT_MAX
        elif bar == "pre_l2":
            pre = _uniform(stored, 1.1 * P.FP32_PRE_L2)
        elif bar == "pre_max":
            pre[1, 3, 5] += 1.1 * P.FP32_PRE_MAX / SC
        elif bar == "out_l2":
            out = _uniform(sh, 1.1 * P.FP32_OUT_L2)
        elif bar == "out_max":
            out[2, 7, 9] -= 1.1 * P.FP32_OUT_MAX
    else:
        if bar is None:
            pre = _one_step(stored, _some(stored, 0.9 * P.FP16_PRE_DIFF_FRAC))
            m = _some(sh, 0.9 * P.FP16_OUT_DIFF_FRAC)
            out = sh + m * _signs(sh) * 0.85 * P.FP16_OUT_L2 * np.linalg.norm(sh) / np.sqrt(m.sum())
            first = np.unravel_index(np.flatnonzero(m)[0], m.shape)
            out[first] = sh[first] + 0.95 * P.FP16_OUT_MAX
        elif bar == "pre_ulp":
            pre[1, 3, 5] += 2 * P.half_ulp(stored[1, 3, 5])             # (two steps by the predicate's own measure)
        elif bar == "pre_diff_frac":
            pre = _one_step(stored, _some(stored, 1.2 * P.FP16_PRE_DIFF_FRAC))
        elif bar == "out_l2":
            out = sh + _some(sh, 0.75 * P.FP16_OUT_DIFF_FRAC) * _signs(sh) * 0.85 * P.FP16_OUT_MAX
        elif bar == "out_max":
            out[2, 7, 9] += 1.1 * P.FP16_OUT_MAX
        elif bar == "out_diff_frac":
            out = _one_step(sh, _some(sh, 1.2 * P.FP16_OUT_DIFF_FRAC))
    return pre, out


def _parity(precision, pre, out, ref, **kw):
    P.assert_parity("synthetic p%d" % precision, precision, pre, out, ref["y"], SC, U, **kw)


@pytest.mark.parametrize("precision", [0, 2])
def test_a_pair_just_inside_every_bar_passes(precision, ref, capsys):
    pre, out = _pair(precision, None, ref)
    assert _violated(precision, pre, out, ref) == []
    _parity(precision, pre, out, ref)
    line = capsys.readouterr().out
    assert line.startswith("MEASURED synthetic p%d: pre_" % precision) and "last_row_max" in line
    figs = dict(zip(line.split(": ")[1].split()[::2], map(float, line.split(": ")[1].split()[1::2])))
    # "just inside": every printed figure that has a bar sits above 0.7 of it
    bars = ({"pre_l2": P.FP32_PRE_L2, "pre_max": P.FP32_PRE_MAX, "out_l2": P.FP32_OUT_L2, "out_max": P.FP32_OUT_MAX} if precision == 0 else
            {"pre_diff_frac": P.FP16_PRE_DIFF_FRAC, "out_l2": P.FP16_OUT_L2, "out_max": P.FP16_OUT_MAX, "out_diff_frac": P.FP16_OUT_DIFF_FRAC})
    for k, bar in bars.items():
        assert 0.7 * bar <= figs[k] <= bar, (k, figs[k], bar)
    assert precision == 0 or 0.5 < figs["pre_max_ulps"] <= 1.0


@pytest.mark.parametrize("precision,bar", [(0, b) for b in P0_BARS] + [(2, b) for b in P2_BARS])
def test_each_bar_alone_makes_it_raise(precision, bar, ref):
    pre, out = _pair(precision, bar, ref)
    assert _violated(precision, pre, out, ref) == [bar]
    with pytest.raises(AssertionError):
        _parity(precision, pre, out, ref)


@pytest.mark.parametrize("precision", [0, 2])
def test_the_last_row_is_compared(precision, ref):
    """an error in the last output row and nowhere else: the rows above meet every bar, the image does not"""
    pre, sh = ref[precision]
    out = sh.copy()
    out[0, -1, 11] += 1.1 * (P.FP32_OUT_MAX if precision == 0 else P.FP16_OUT_MAX)
    assert np.array_equal(out[:, :-1], sh[:, :-1])
    assert _violated(precision, pre, out, ref) == ["out_max"]
    with pytest.raises(AssertionError):
        _parity(precision, pre, out, ref)


def test_pooled_mode_takes_the_counts_in_place_of_the_fraction_bars(ref):
    stored, sh = ref[2]
    pre, _ = _pair(2, "pre_diff_frac", ref)
    _, out = _pair(2, "out_diff_frac", ref)
    assert _violated(2, pre, out, ref) == ["out_diff_frac", "pre_diff_frac"]
    acc = []
    assert P.assert_parity("pooled", 2, pre, out, ref["y"], SC, U, pooled=acc) is None
    assert acc == [(int((pre != stored).sum()), pre.size, int((out != sh).sum()), out.size)]
    assert acc[0][0] > P.FP16_PRE_DIFF_FRAC * pre.size and acc[0][2] > P.FP16_OUT_DIFF_FRAC * out.size
    with pytest.raises(AssertionError):
        P.pooled_fraction_bars("pooled", acc)


@pytest.mark.parametrize("counts,ok", [([(100, 10000, 200, 10000)], True), ([(60, 5000, 0, 5000), (41, 5000, 0, 5000)], False),
                                       ([(0, 5000, 101, 5000), (0, 5000, 100, 5000)], False), ([(101, 10000, 201, 10000)], False)])
def test_pooled_fraction_bars(counts, ok):
    if ok:
        P.pooled_fraction_bars("pooled", counts)
    else:
        with pytest.raises(AssertionError):
            P.pooled_fraction_bars("pooled", counts)


@pytest.mark.parametrize("bar", ["pre_ulp", "out_l2", "out_max"])
def test_the_per_case_bars_hold_in_pooled_mode(bar, ref):
    pre, out = _pair(2, bar, ref)
    acc = []
    with pytest.raises(AssertionError):
        _parity(2, pre, out, ref, pooled=acc)
    assert acc == []


@pytest.mark.parametrize("precision,pre_bar,out_bar", [(0, "pre_max", "out_max"), (2, "pre_ulp", "out_diff_frac")])
def test_without_pre_the_output_alone_is_checked(precision, pre_bar, out_bar, ref, capsys):
    pre, out = _pair(precision, pre_bar, ref)
    with pytest.raises(AssertionError):
        _parity(precision, pre, out, ref)
    capsys.readouterr()
    _parity(precision, None, out, ref)
    line = capsys.readouterr().out
    assert "pre_" not in line and "out_l2" in line and "last_row_max" in line
    # (the output as the device hands it over: the plan's storage type)
    _parity(precision, None, out.astype(np.float32 if precision == 0 else np.float16), ref)
    with pytest.raises(AssertionError):
        _parity(precision, None, _pair(precision, out_bar, ref)[1], ref)


def test_identity_bars(ref):
    x = ref[0][0]
    inside = _uniform(x, 0.9 * P.FP32_PRE_L2)
    inside[0, 0, 0] = x[0, 0, 0] + 0.95 * P.FP32_PRE_MAX
    P.assert_identity("identity", inside, x)
    one = x.copy()
    one[2, -1, -1] += 1.1 * P.FP32_PRE_MAX
    assert P.rel_l2(one, x) <= P.FP32_PRE_L2
    with pytest.raises(AssertionError):
        P.assert_identity("identity", one, x)
    everywhere = _uniform(x, 1.1 * P.FP32_PRE_L2)
    assert np.abs(everywhere - x).max() <= P.FP32_PRE_MAX
    with pytest.raises(AssertionError):
        P.assert_identity("identity", everywhere, x)


def test_primitives(capsys):
    P.measured("tag 3x4", a=1.23456e-5, b=2)
    assert capsys.readouterr().out == "MEASURED tag 3x4: a 1.23e-05  b 2\n"
    assert P.rel_l2(np.array([3.0, 4.0]), np.array([3.0, 0.0])) == pytest.approx(4.0 / 3.0)
    assert [n for n in range(-1, 17) if P.smooth(n)] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16]
    # one ulp of binary16: 2^-10 |x| for normal numbers, 2^-24 below 2^-14
    x = np.array([1.0, -0.75, 2.0 ** -14, 2.0 ** -20, 0.0])
    assert np.array_equal(P.half_ulp(x), [2.0 ** -10, 0.75 * 2.0 ** -10, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24])
    assert P.within_one_half_ulp(x + P.half_ulp(x), x).all() and not P.within_one_half_ulp(x + 2 * P.half_ulp(x) + 1e-6, x).any()
