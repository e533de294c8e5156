"""CPU suite: the case lists of the family sweeps (tests/family_sweep_cases.py) against the planner itself and against the oracles.

tests/plan_rules_driver.cpp (built as in tests/test_host_plan_rules.py, device facts of an MI355X from
tests/golden/plan_geometry.json) answers EVERY case of every arm at the default seed and count and at two other seeds.  No answer
may be an error: the GPU sweep (tests/test_gpu_family_sweep.py) has no skip path, and a case the planner refuses is a bug of the
generator.  Every stratum the generator promises is then read off the planner's decisions (TK, NT, ncols, bzL, viewL, ldsCol, align,
exact, down, dct ...) and off the case tuples, one assertion per stratum with its name in the message -- for all three seeds, so
that the coverage is the forced part's and not luck.

The oracles at the shapes the GPU is judged at: for every exact and view case whose four lengths are at most 64, the FFT statement
of the exact-size oracle against its dense-matrix statement, and the view oracle against the exact-size oracle where the view is a
full frame, to 1e-12 (the bar tests/test_gpu_view.py uses between two oracles)."""
import numpy as np
import pytest

import dct_oracle as D
import exactsize_oracle as E
import family_sweep_cases as F
import plan_driver
import view_oracle as V
import vkresample_amd as v

FAMILY = {"generic": 0, "dct": 6, "down": 7, "odd": 8, "view": 9}
SEEDS = [None, 1, 987654321]           # None: FFTUP_SWEEP_SEED or its default


def request(arm, c, precision):
    if arm == "exact":
        W, H, uW, uH, align, any_flag = c
        return plan_driver.request_line("size", W, H, 1.0, precision, v.FLAG_ANY_SIZE if any_flag else 0, 0, (uW, uH), align)
    if arm == "odd":
        W, H, u, extra = c
        flags = v.FLAG_ODD_SIZE | (v.FLAG_ANY_SIZE if "any" in extra else 0) | (v.FLAG_DOWNSCALE if "down" in extra else 0)
        return plan_driver.request_line("create", W, H, u, precision, flags)
    if arm == "any":
        W, H, u, down = c
        return plan_driver.request_line("create", W, H, u, precision, v.FLAG_ANY_SIZE | (v.FLAG_DOWNSCALE if down else 0))
    if arm == "down":
        W, H, u, dct = c
        return plan_driver.request_line("create", W, H, u, precision, v.FLAG_DOWNSCALE | (v.FLAG_DCT if dct else 0))
    if arm == "dct":
        W, H, u = c
        return plan_driver.request_line("create", W, H, u, precision, v.FLAG_DCT)
    W, H, uW, uH, origin, span, any_flag = c
    return plan_driver.request_line("view", W, H, 1.0, precision, v.FLAG_ANY_SIZE if any_flag else 0, 0, (uW, uH), 0, tuple(origin) + tuple(span))


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """{seed: {arm: [(case, precision, fields of the planner's answer or the error line)]}}"""
    d = tmp_path_factory.mktemp("family_sweep")
    exe = plan_driver.build(d)
    out = {}
    for s in SEEDS:
        lines, index = [], []
        for arm in F.ARMS:
            cases = F.CASES[arm](s=s)
            for c, (p, _) in zip(cases, F.precision_and_input(arm, len(cases), s)):
                lines.append(request(arm, c, p))
                index.append((arm, c, p))
        got = plan_driver.run(exe, d, lines)
        out[s] = {arm: [] for arm in F.ARMS}
        for (arm, c, p), line in zip(index, got):
            out[s][arm].append((c, p, line if line.startswith("error") else plan_driver.fields(line)))
    return out


def _ints(text):
    return [int(x) for x in text.split(",")]


@pytest.mark.parametrize("s", SEEDS)
def test_every_case_is_a_valid_request_of_its_own_family(planned, s):
    for arm in F.ARMS:
        rows = planned[s][arm]
        assert len(rows) >= F.DEFAULT_N[arm] or len(rows) == F.count(arm)
        for c, p, g in rows:
            assert not isinstance(g, str), "%s %r: the planner refuses it: %s" % (arm, c, g)
            want = {"exact": "odd", "odd": "odd", "any": "down" if arm == "any" and c[3] else "generic",
                    "down": "dct" if arm == "down" and c[3] else "down", "dct": "dct", "view": "view"}[arm]
            assert int(g["family"]) == FAMILY[want], "%s %r: family %s" % (arm, c, g["family"])


def test_default_counts_hold_the_strata_and_a_random_part():
    forced = {"exact": F.exact_forced, "odd": F.odd_forced, "any": F.any_forced, "down": F.down_forced, "dct": F.dct_forced, "view": F.view_forced}
    for arm in F.ARMS:
        assert len(forced[arm]()) < F.DEFAULT_N[arm] < F.BIG_N[arm], arm
        assert F.CASES[arm](n=1)[:len(forced[arm]())] == forced[arm](), arm + ": a small count never cuts the strata"
        assert len(set(F.CASES[arm](n=F.BIG_N[arm]))) == F.BIG_N[arm], arm
    assert F.DEFAULT_N["odd"] < F.DEFAULT_N["exact"]


def test_precision_and_input_are_balanced():
    for arm in F.ARMS:
        for n in (F.DEFAULT_N[arm], F.BIG_N[arm]):
            pairs = F.precision_and_input(arm, n)
            for want in ((0, False), (0, True), (2, False), (2, True)):
                assert pairs.count(want) >= n // 4, (arm, n, want)


@pytest.mark.parametrize("s", SEEDS)
def test_strata_exact(planned, s):
    rows = planned[s]["exact"]
    dev = plan_driver.golden_rows("plan_geometry.json")["device"]
    for c, _, g in rows:
        assert (g["exact"], g["odd"], int(g["align"])) == ("1", "1", c[4]) and (int(g["uW"]), int(g["uH"])) == (c[2], c[3]), c
    for axis, (n, m) in (("rows", (0, 2)), ("columns", (1, 3))):
        seen = {F.axis_class(c[n], c[m]) + (c[4],) for c, _, _ in rows}
        for cls in F.AXIS_CLASSES:
            if cls[2] == "equal":                          # (M = N: the alignments are the same map)
                assert cls + (0,) in seen or cls + (1,) in seen, "exact: class %s on %s" % (cls, axis)
                continue
            for align in (0, 1):
                assert cls + (align,) in seen, "exact: class %s on %s at alignment %d" % (cls, axis, align)
    for pos, name in enumerate(("W", "H", "uW", "uH")):
        for length in (2, 3):
            assert any(c[pos] == length for c, _, _ in rows), "exact: a length of %d as %s" % (length, name)
        others = [i for i in range(4) if i != pos]
        assert any(not F.smooth(c[pos]) and all(F.smooth(c[i]) for i in others) and _ints(g["bzL"])[pos] for c, _, g in rows), \
            "exact: a non-smooth length as %s alone" % name
    assert {4, 5, 7, 8} <= {x for c, _, _ in rows for x in c[:4]}, "exact: the single-stage lengths 4, 5, 7, 8"
    assert any(all(_ints(g["bzL"])) and len(set(_ints(g["bzL"]))) >= 3 for _, _, g in rows), "exact: four Bluestein transforms with at least three lengths L"
    tight = {c[i] for c, _, g in rows for i in range(4) if _ints(g["bzL"])[i] == 2 * c[i] - 1 and all(c[i] % q for q in range(2, c[i]))}
    assert len(tight) >= 2, "exact: two primes whose Bluestein length is 2N - 1 itself (%s)" % sorted(tight)
    res = {int(g["ncols"]) % 8 for c, _, g in rows if g["TK"] == "8" and int(g["ncols"]) == min(c[0], c[2]) // 2 + 1}
    assert res == set(range(8)), "exact: every residue of min(W, uW)/2 + 1 modulo 8 at TK 8 (%s)" % sorted(res)
    for tk in ("4", "2", "1"):
        assert any(g["TK"] == tk and (_ints(g["bzL"])[1] or _ints(g["bzL"])[3]) for _, _, g in rows), "exact: TK %s under the Bluestein rule" % tk
    assert any(g["TK"] != "8" and _ints(g["bzL"])[1] and _ints(g["bzL"])[3] for _, _, g in rows), "exact: a thin frame with a Bluestein transform on both column lengths"
    assert any(g["TK"] != "8" and _ints(g["bzL"])[1] and not _ints(g["bzL"])[3] and c[3] < c[1] for c, _, g in rows), \
        "exact: a thin frame with a Bluestein transform on H and a smaller smooth uH (a crop beside it)"
    assert any(0 <= dev["lds_bytes"] - int(g["ldsCol"]) < 1024 for _, _, g in rows), "exact: column LDS within 1 KB of the device limit"
    assert any(c[4] == 1 and ((c[2] < c[0] and c[2] % 2 == 0) or (c[3] < c[1] and c[3] % 2 == 0)) for c, _, _ in rows), "exact: a folded Nyquist bin at centre alignment"
    assert any(c[4] == 1 and ((c[2] > c[0] and c[0] % 2 == 0) or (c[3] > c[1] and c[1] % 2 == 0)) for c, _, _ in rows), "exact: a split Nyquist bin at centre alignment"


@pytest.mark.parametrize("s", SEEDS)
def test_strata_odd(planned, s):
    rows = planned[s]["odd"]
    for c, p, g in rows:
        lens = [int(g[k]) for k in ("W", "H", "uW", "uH")]
        assert g["odd"] == "1" and g["exact"] == "0" and any(x & 1 for x in lens), c
        assert lens[2:] == [F.out_size(c[0], c[2]), F.out_size(c[1], c[2])], "odd: the fp32 size rule of %r" % (c,)
        assert float.fromhex(g["upsq"]) == D.upsq(c[2], p == 2), "odd: upsq from cfg->upscale of %r" % (c,)
        assert (g["down"] == "1") == ("down" in c[3]) == (c[2] < 1.0), c
    ups = {c[2] for c, _, _ in rows}
    for u in F.JIT_FACTORS:
        assert float(np.float32(u)) in ups, "odd: the factor %g" % u
    assert len({c[2] for c, _, _ in rows if c[2] < 1.0}) >= 8, "odd: downscale reciprocals of the factors"
    assert any(g["bz"] == "1" for _, _, g in rows) and any(g["bz"] == "0" for _, _, g in rows), "odd: with and without FFTUP_FLAG_ANY_SIZE"
    assert any(g["bz"] == "1" and g["down"] == "1" for _, _, g in rows), "odd: FFTUP_FLAG_ANY_SIZE together with FFTUP_FLAG_DOWNSCALE"


@pytest.mark.parametrize("s", SEEDS)
def test_strata_any(planned, s):
    rows = planned[s]["any"]
    for c, _, g in rows:
        lens = [int(g[k]) for k in ("W", "H", "uW", "uH")]
        assert g["bz"] == "1" and g["odd"] == "0" and not any(x & 1 for x in lens), c
        assert (g["down"] == "1") == c[3], c
        if not c[3]:
            assert (int(g["zly"]), int(g["zry"])) == (c[1] // 2, lens[3] - c[1] // 2), "any: the symmetric zero-padding range of %r" % (c,)
    for pos, name in enumerate(("W", "H", "uW", "uH")):
        assert any(_ints(g["bzL"])[pos] for _, _, g in rows), "any: a non-smooth length as %s" % name
    for u in F.ANY_UP:
        assert any(c[2] == u for c, _, _ in rows), "any: the factor %g" % u
    assert any(c[3] for c, _, _ in rows), "any: a downscale factor with FFTUP_FLAG_DOWNSCALE"
    for tk in ("4", "2", "1"):
        assert any(g["TK"] == tk and g["poly"] == "0" for _, _, g in rows), "any: TK %s under the Bluestein rule" % tk
    res = {int(g["ncols"]) % 8 for _, _, g in rows if g["TK"] == "8"}
    assert res == set(range(8)), "any: every residue of ncols modulo 8 at TK 8 (%s)" % sorted(res)


@pytest.mark.parametrize("s", SEEDS)
def test_strata_down(planned, s):
    rows = planned[s]["down"]
    for c, _, g in rows:
        lens = [int(g[k]) for k in ("W", "H", "uW", "uH")]
        assert all(F.smooth(x) and x % 2 == 0 and x >= 2 for x in lens) and lens[2] < lens[0] and lens[3] < lens[1], c
        assert g["down"] == "1" and (g["dct"] == "1") == c[3] and g["bz"] == "0" and g["odd"] == "0", c
    for u in F.DOWN_FACTORS:
        assert any(c[2] == float(np.float32(u)) and not c[3] for c, _, _ in rows), "down: the factor %g" % u
    assert sum(1 for c, _, _ in rows if c[3]) >= 4, "down: FFTUP_FLAG_DOWNSCALE | FFTUP_FLAG_DCT"
    for dct in (False, True):
        assert any(c[3] == dct and 2 in (int(g["uW"]), int(g["uH"])) for c, _, g in rows), "down: an output length of 2 (dct %d)" % dct
    res = {int(g["ncols"]) % 8 for c, _, g in rows if not c[3] and g["TK"] == "8" and int(g["ncols"]) == int(g["uW"]) // 2 + 1}
    assert res == set(range(8)), "down: every residue of uW/2 + 1 modulo 8 (%s)" % sorted(res)


@pytest.mark.parametrize("s", SEEDS)
def test_strata_dct(planned, s):
    rows = planned[s]["dct"]
    for c, _, g in rows:
        assert g["dct"] == "1" and g["down"] == "0" and (int(g["uW"]), int(g["uH"])) == (F.out_size(c[0], c[2]), F.out_size(c[1], c[2])), c
        assert (c[0] in F.DCT_SMOOTH or c[0] == 2) and (c[1] in F.DCT_SMOOTH or c[1] == 2), c
    for u in F.DCT_FACTORS:
        assert any(c[2] == u for c, _, _ in rows), "dct: the factor %g" % u
    for pos, name in enumerate(("W", "H")):
        for length in (2, 4):
            assert any(c[pos] == length for c, _, _ in rows), "dct: an input length of %d as %s" % (length, name)
    assert any(c[2] == 1.0 and min(c[0], c[1]) >= 16 for c, _, _ in rows), "dct: the identity, u = 1"


def _prime(n):
    return n > 1 and all(n % q for q in range(2, int(n ** 0.5) + 1))


@pytest.mark.parametrize("s", SEEDS)
def test_strata_view(planned, s):
    rows = planned[s]["view"]
    for c, _, g in rows:
        assert g["view"] == "1" and (int(g["uW"]), int(g["uH"])) == (c[2], c[3]), c
    axes = [(c[0 + a], c[2 + a], c[4][a], c[5][a]) for c, _, _ in rows for a in (0, 1)]               # (N, M, origin, span)
    for a, name in enumerate(("x", "y")):
        ax = [(c[0 + a], c[2 + a], c[4][a], c[5][a]) for c, _, _ in rows]
        assert any(sp / M == 8.0 for _, M, _, sp in ax), "view: step exactly 8 on " + name
        assert any(sp / M == 1.0 / 64 for _, M, _, sp in ax), "view: step exactly 1/64 on " + name
        assert any(8.0 * (1 - 1e-6) < sp / M < 8.0 for _, M, _, sp in ax), "view: step just below 8 on " + name
        assert any(1.0 / 64 < sp / M < (1 + 1e-6) / 64 for _, M, _, sp in ax), "view: step just above 1/64 on " + name
    assert any(sp == M and N % 2 == 0 and V.kmax(N, M, sp) == N // 2 for N, M, _, sp in axes), "view: step 1 on an even N: kmax = N/2, the Nyquist bin at weight 1/2"
    assert any(sp == M and N % 2 == 1 and V.kmax(N, M, sp) == (N - 1) // 2 for N, M, _, sp in axes), "view: step 1 on an odd N: kmax = (N - 1)/2"
    assert any(M < sp < M * (1 + 1e-3) and V.kmax(N, M, sp) == V.kmax(N, M, M) - 1 for N, M, _, sp in axes), "view: a step just above 1 that drops one bin"
    assert any(o < 0 for _, _, o, _ in axes) and any(o > N for N, _, o, _ in axes), "view: origins left of the frame and beyond it"
    assert any(_ints(g["bzL"])[0] for _, _, g in rows) and any(_ints(g["bzL"])[1] for _, _, g in rows), "view: a non-smooth W and a non-smooth H"
    assert any(_prime(c[2]) and c[2] > 7 for c, _, _ in rows) and any(_prime(c[3]) and c[3] > 7 for c, _, _ in rows), "view: prime output lengths"
    assert any(N == 2 and M >= 32 for N, M, _, _ in axes) and any(M == 2 and N >= 32 for N, M, _, _ in axes), "view: N = 2 under a large M, M = 2 over a large N"
    for tk in ("4", "2", "1"):
        assert any(g["TK"] == tk for _, _, g in rows), "view: TK %s under the view rule" % tk
    assert any(_ints(g["bzL"])[1] == 8192 and _ints(g["viewL"])[1] == 8192 for _, _, g in rows), "view: a Bluestein forward column and a convolution, both of length 8192"


def _planes(W, H, k):
    return np.random.RandomState(1000 + k).rand(3, H, W)


def test_exact_oracle_fft_statement_agrees_with_its_matrices():
    n = 0
    for k, (W, H, uW, uH, align, _) in enumerate(F.exact_cases()):
        if max(W, H, uW, uH) > 64:
            continue
        x = _planes(W, H, k)
        Rx, Ry = E.resample_matrix(W, uW, align), E.resample_matrix(H, uH, align)
        dense = Ry @ x @ Rx.T
        assert np.abs(dense.imag).max() <= 1e-12 and np.abs(E.resample_R(x, uW, uH, align) - dense.real).max() <= 1e-12, (W, H, uW, uH, align)
        n += 1
    assert n >= 30


def test_view_oracle_agrees_with_the_exact_size_oracle_on_full_frames():
    n = 0
    for k, (W, H, uW, uH, origin, span, _) in enumerate(F.view_cases()):
        if max(W, H, uW, uH) > 64 or tuple(span) != (float(W), float(H)):
            continue
        for align in (E.ALIGN_CORNER, E.ALIGN_CENTRE):
            if tuple(origin) == (E.delta(W, uW, align), E.delta(H, uH, align)):
                x = _planes(W, H, k)
                assert np.abs(V.view_planes(x, uW, uH, origin, span) - E.resample_planes(x, uW, uH, align)).max() <= 1e-12, (W, H, uW, uH, align)
                n += 1
                break
    assert n >= 2
