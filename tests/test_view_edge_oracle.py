"""CPU: everything tests/test_gpu_view_edges.py takes for granted, proven on the fp64 oracles (tests/view_oracle.py,
tests/mirror_oracle.py) and the device-free planner (tests/plan_driver.py) alone -- every literal of tests/view_edge_cases.py
recomputed (kmax and L by the oracles' rules, TK and the accept / reject pair around the largest column convolution through the
library's own plan rules), the oracles held to their chirp-z factorisation in long double at the edges, the far origins reduced,
and the probes shown to tell a plan that is one bin off from a right one."""
import numpy as np
import pytest

import mirror_oracle as Mo
import paritylib as P
import plan_driver as PD
import view_edge_cases as EC
import view_oracle as V

TOL = 1e-9                   # of full scale: the inputs lie in [0, 1]


def test_kmax_and_L_literals():
    """every kmax and L of the table by the oracles' rules; the mirror rows' kmax is the tables' (N: the zero bin), one above the
    last cosine where the cap holds"""
    assert len(set(EC.NAMES)) == len(EC.NAMES)
    for r in EC.ROWS:
        assert EC.recomputed(r) == tuple(r[8:12]), (r[0], EC.recomputed(r))
        for axis, (N, M, _, span) in enumerate(EC.axes(r)):
            K = 2 * r[8 + axis] + 1
            assert r[10 + axis] >= K + M - 1                            # (the two wings of the chirp do not meet)
            assert 1.0 / 64 <= span / M <= 8.0
            if EC.mirror(r):
                assert Mo.kmax(N, M, span) == min(r[8 + axis], N - 1)


def test_the_rows_sit_on_their_edges():
    """the hand-stated edges, so that a changed shape cannot quietly leave its edge"""
    R = {r[0]: r for r in EC.ROWS}
    # tiles: max(L_y, a Bluestein forward length) TK fits the two buffers, twice the tile does not; W = 8 leaves the last tile partial
    for name, tk in EC.TK_OF.items():
        r = R[name]
        longest = max(r[11], EC.TK2_BZ_FORWARD if name == "tk2_bz" else 0)
        assert r[12] == tk and longest * tk <= EC.LDS_POINTS and (tk == 8 or longest * 2 * tk > EC.LDS_POINTS), name
        ncols = (r[1] // 2 + 1) if EC.mirror(r) and r[8] >= r[1] // 2 else r[8] + 1
        assert ncols % tk != 0 or tk == 1, name
    assert all(r[12] == 8 for r in EC.ROWS if r[0] not in EC.TK_OF)
    assert R["tk4_trunc"][8] + 1 == 2 < 4 and R["tk4_trunc"][6][0] / 8 > 2
    assert not P.smooth(1306) and V.smooth_from(2 * 1306 - 1) == EC.TK2_BZ_FORWARD > R["tk2_bz"][11] and R["tk2_bz"][11] * 4 <= EC.LDS_POINTS
    assert R["tk2"][7] & EC.U8 and R["tk4_m"][7] & EC.U8
    # the largest column convolution: 9604 is the last smooth length that fits, 9720 the next one
    lp = lambda n: n + n // 16 + 1
    assert 16 * lp(EC.LDS_POINTS) <= 160 * 1024 < 16 * lp(EC.LDS_POINTS + 1)
    assert V.smooth_from(9605) == 9720 > EC.LDS_POINTS >= 9604 == R["ymax"][11] == R["ymax_m"][11]
    for name, W, H, uW, uH, span, flags, Ly in EC.REJECTED:
        assert (Mo.conv_length(H, uH) if flags & EC.MIRROR else V.conv_length(H, uH)) == Ly == 9720
    # steps at the closed bounds, the other axis near 1
    for name, axis, step in (("step64", 0, 1.0 / 64), ("step64_m", 0, 1.0 / 64), ("step8", 1, 8.0), ("step8_m", 1, 8.0), ("k0", 0, 8.0), ("k0_y", 1, 8.0), ("k0_m", 0, 8.0)):
        ax = EC.axes(R[name])
        assert ax[axis][3] / ax[axis][1] == step and 0.9 <= ax[1 - axis][3] / ax[1 - axis][1] <= 1.25, name
    assert R["k0"][8] == 0 and R["k0_y"][9] == 0 and R["k0_m"][8] == 0 and R["k0"][1] == 8 == R["k0_y"][2]
    # (k0, k0_m: y is a quarter-pixel shift at step 1, the identity in mean_view; k0_y the same with the axes swapped)
    assert EC.axes(R["k0"])[1] == (12, 12, 0.25, 12.0) == EC.axes(R["k0_m"])[1] and EC.axes(R["k0_y"])[0] == (12, 12, 0.25, 12.0)
    assert EC.axes(EC.mean_view(R["k0"], 2))[1] == (12, 12, 0.0, 12.0) == EC.axes(EC.mean_view(R["k0_y"], 1))[0]
    assert EC.mean_view(R["k0_m"], 2)[6:] == R["k0_m"][6:] and [n for n, _ in EC.K0_ROWS] == ["k0", "k0_m", "k0_y"]
    # the floor: N M / (2 span) (mirror: N M / span) is an integer in the _lo row, and the _hi row is the next double
    for lo, hi in EC.PROBE_PAIRS + (("mirror_cap", "mirror_cap_hi"),):
        a, b = R[lo], R[hi]
        assert a[1:6] == b[1:6] and a[7] & ~EC.U8 == b[7] & ~EC.U8
        for axis in (0, 1):
            N, M, _, span = EC.axes(a)[axis]
            q = N * M / span if EC.mirror(a) else N * M / (2 * span)
            assert q == int(q) == a[8 + axis] == b[8 + axis] + 1 and EC.axes(b)[axis][3] == np.nextafter(span, np.inf), (lo, axis)
    for axis in (0, 1):
        N, M, _, span = EC.axes(R["nyq_kept"])[axis]
        assert N % 2 == 0 and span == M and R["nyq_kept"][8 + axis] == N // 2
        N, M, _, span = EC.axes(R["mirror_cap"])[axis]
        assert span == M and R["mirror_cap"][8 + axis] == N and Mo.kmax(N, M, span) == N - 1 == Mo.kmax(N, M, np.nextafter(span, np.inf))
        N, M, _, span = EC.axes(R["mcap_lo"])[axis]
        assert R["mcap_lo"][8 + axis] == N - 1 == Mo.kmax(N, M, span)
    # far origins; reflected copies
    assert R["far"][5] == R["far_m"][5] == (1e9 + 0.37, -1e9 - 0.61)
    assert R["farther"][5] == R["farther_m"][5] == (2.0 ** 49 + 0.375, -2.0 ** 49 - 0.625) and R["farther"][5][0] - 2.0 ** 49 == 0.375
    for (N, M, origin, span) in EC.axes(R["far_refl_m"]):
        assert span > 2 * N and origin < -N
    # the smallest lengths: K = 3 with both end bins the half-weighted Nyquist bin, L = 4
    assert R["min2"][1:5] == (2, 2, 2, 2) == R["min2_m"][1:5] and R["min3"][1:5] == (3, 2, 2, 3)
    assert R["min2"][8:12] == (1, 1, 4, 4) and R["min2"][5] == (0.25, 0.5)
    # the per-frame calls: every name is a row of the calls' shape
    for m in (False, True):
        for lanes in (3, 1):
            names = EC.frame_views(m, lanes)
            assert len(set(names)) == len(names)
            for lo, hi in (("kflip_lo", "kflip_hi"), ("nyq_kept", "nyq_dropped")) if not m else (("kflip_lo_m", "kflip_hi_m"), ("mirror_cap", "mirror_cap_hi")):
                assert names.index(hi) - names.index(lo) == lanes            # (consecutive frames on one lane)
        assert set(EC.FRAME_VIEWS[m]) == set(EC.FRAME_VIEWS_ONE_LANE[m])
        last = EC.last_on_lane(EC.FRAME_VIEWS[m], 3)
        assert EC.FRAME_VIEWS[m][last[2]].startswith("kflip_hi") and EC.FRAME_VIEWS[m][last[1]].startswith("far")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("view_edges_plan")
    exe = PD.build(d)
    return lambda lines: PD.run(exe, d, lines)


def _request(W, H, uW, uH, origin, span, flags, precision):
    return PD.request_line("view", W, H, 1.0, precision, flags, 0, (uW, uH), 0, tuple(origin) + tuple(span))


def test_tile_widths_and_the_largest_column_through_the_planner(planner):
    """TK, L and the spectrum columns of every row from the library's own rules, -p 0 and -p 2, with and without the 8-bit load;
    the two rejected shapes come back FFTUP_E_UNSUPPORTED_SIZE (2) over their columns.  This is what proves that tk4, tk2 and tk1
    select the instantiations of k_col_view they are named after."""
    lds_max = PD.golden_rows("plan_geometry.json")["device"]["lds_bytes"]
    runs = [(r, p, u8) for r in EC.ROWS for p in (0, 2) for u8 in ((False, True) if EC.runs_u8(r) else (False,))]
    out = planner([_request(*r[1:7], EC.plan_flags(r, u8), p) for r, p, u8 in runs])
    for (r, p, u8), line in zip(runs, out):
        assert not line.startswith("error"), (r[0], line)
        g = PD.fields(line)
        assert int(g["TK"]) == r[12], (r[0], g["TK"])
        assert g["viewL"] == "%d,%d" % (r[10], r[11]) and g["view"] == "1", (r[0], g["viewL"])
        assert int(g["ldsCol"]) <= lds_max and int(g["ldsCol"]) >= 16 * r[11] * r[12]
        assert g["ncols"] == str(r[1] // 2 + 1)                         # (the buffers' worst case; the view's own count: below)
        bz = [int(t) for t in g["bzL"].split(",")]
        assert (bz[1] != 0) == (not P.smooth(r[2])) and (r[0] != "tk2_bz" or bz[1] == EC.TK2_BZ_FORWARD), (r[0], bz)
    rej = planner([_request(W, H, uW, uH, (0.0, 0.0), span, flags, p) for (_, W, H, uW, uH, span, flags, _) in EC.REJECTED for p in (0, 2)])
    for line in rej:
        assert line.startswith("error 2 ") and "columns" in line, line


# ------------------------------------------------------------------------------------------------- the oracle holds at the edges
def _axes_up_to(limit):
    """the distinct (mirror, N, M, origin, span) of the table whose N and M are at most `limit`"""
    seen = []
    for r in EC.ROWS:
        for ax in EC.axes(r):
            if max(ax[0], ax[1]) <= limit and (EC.mirror(r),) + ax not in seen:
                seen.append((EC.mirror(r),) + ax)
    return seen


def test_dense_statement_against_the_chirp_factorisation_in_longdouble():
    """both axes of every row up to DENSE_LIMIT points: the dense matrix (at the origin reduced in fp64, as the GPU test uses it)
    against the chirp-z factorisation in long double AT THE ORIGIN ITSELF (its tables reduce the origin in long double, where
    fmodl is exact as well) -- 1e-9 of full scale.  For the far rows this is the statement that the reduction changes nothing."""
    worst, count = 0.0, 0
    for m, N, M, origin, span in _axes_up_to(EC.DENSE_LIMIT):
        x = np.random.default_rng(N + M).random(N)
        A, B = EC.factors(N, M, float(origin), float(span), m)
        dense = np.real((A @ B) @ x)
        assert np.abs(np.imag(A @ B)).max() <= 1e-12
        chirp = (Mo.mirror_1d_chirp if m else V.view_1d_chirp)(x, M, origin, span)
        err = max(np.abs(chirp.real - dense).max(), np.abs(chirp.imag).max())
        worst, count = max(worst, err), count + 1
        assert err <= TOL, (m, N, M, origin, span, err)
        assert np.abs((A @ B).sum(axis=1) - 1.0).max() <= TOL                  # constants stay constant
    print("MEASURED view edges: dense vs long double chirp over %d axes, worst %.3g" % (count, worst))
    assert count >= 40
    assert {(m, N, M) for m, N, M, _, _ in _axes_up_to(EC.DENSE_LIMIT)} >= {(False, 2, 2), (False, 3, 2), (False, 2, 3), (True, 2, 2), (False, 8, 6), (True, 4, 6)}


def test_far_origins_reduce_exactly():
    """fmod(origin, period) in fp64 is the origin up to a whole number of periods -- exactly: the difference, formed in long
    double, is an integer multiple of the period.  And the dense statement at the unreduced 1e9, which reduces nothing, agrees as
    far as fp64 lets it: its positions origin + m s are rounded to ulp(1e9) / 2 = 6e-8 pixels and the products t f to
    ulp(5e10) / 2 = 4e-6, so a phase 2 pi f t / N is off by up to 2 pi (48 x 6e-8 + 4e-6) / 40 = 1e-6 radians, on the sum of bins
    whose weights a line of values in [0, 1] bounds by a few units -- 1e-5 covers it (measured: 1.5e-7)"""
    ld = np.longdouble
    for name in ("far", "far_m", "far_refl_m", "farther", "farther_m"):
        r = EC.row(name)
        for N, M, origin, span in EC.axes(r):
            period = 2 * N if EC.mirror(r) else N
            o = EC.reduced(origin, N, EC.mirror(r))
            turns = (ld(origin) - ld(o)) / ld(period)
            assert abs(o) < period and turns == np.round(turns) and (abs(origin) < period or turns != 0)
            if abs(origin) > 1e12:                                      # (farther: fp64 has no phase left at the origin itself)
                continue
            x = np.random.default_rng(N).random(N)
            A, B = EC.factors(N, M, float(origin), float(span), EC.mirror(r))
            raw = (Mo.mirror_matrix if EC.mirror(r) else V.view_matrix)(N, M, origin, span)
            assert np.abs(np.real(raw @ x) - np.real(A @ (B @ x))).max() <= (1e-5 if abs(origin) > 1e6 else 1e-12), name


def test_the_shift_oracle_is_the_dense_statement():
    """ymax's oracle (FFTs) against the factors, on a column short enough for both: the same shape of row, 8 x 98 -> 8 x 98"""
    x = np.random.default_rng(7).random((3, 98, 8))
    r = ("short", 8, 98, 8, 98, EC.row("ymax")[5], (8.0, 98.0), 0)
    assert np.abs(V.shift_planes(x, r[5]) - EC.oracle_y(r, x)).max() <= 1e-12
    assert np.abs(EC.oracle_y(r, x) - V.view_planes(x, 8, 98, r[5], r[6])).max() <= 1e-12
    m = EC.row("tk4_m")
    xm = np.random.default_rng(8).random((3, m[2], m[1]))
    assert np.abs(EC.oracle_y(m, xm) - Mo.mirror_planes(xm, m[3], m[4], m[5], m[6])).max() <= 1e-12


# ----------------------------------------------------------------------------------------------------- the probes discriminate
def _probe_outputs(r, axis, k):
    x = EC.probe(r, axis, k).astype(np.float64)
    return EC.oracle_y(r, x)


@pytest.mark.parametrize("lo,hi", EC.PROBE_PAIRS)
def test_probes_tell_the_pair_apart(lo, hi):
    """the cosine at the last frequency the _lo row keeps, along x and along y: the oracle's outputs for the two views differ by at
    least 100 times FP32_PRE_MAX, so a plan that keeps one bin more or one bin fewer than its row cannot meet that bar.  (The
    positions of the two views differ by one ulp of the span: 1e-14 of that.)"""
    a, b = EC.row(lo), EC.row(hi)
    for axis in (0, 1):
        k = EC.last_kept(a, axis)
        assert k == EC.last_kept(b, axis) + 1
        ya, yb = _probe_outputs(a, axis, k), _probe_outputs(b, axis, k)
        gap = np.abs(ya - yb).max()
        print("MEASURED probe %s/%s axis %d k=%d: oracle outputs differ by %.3g" % (lo, hi, axis, k, gap))
        assert gap >= 100 * P.FP32_PRE_MAX
        # the _hi view drops the probe's frequency whole: a constant is left
        assert np.abs(yb - 0.5).max() <= 1e-7                              # (what is left of the fp32 rounding of the probe)
        # a lower frequency passes both views alike
        assert np.abs(_probe_outputs(a, axis, k - 1) - _probe_outputs(b, axis, k - 1)).max() <= 1e-7


def test_mirror_cap_probe_is_the_last_cosine():
    """mirror_cap and mirror_cap_hi keep every cosine the frame has: the DCT-II basis vector k = N - 1 comes back as that cosine at
    the view's positions; the share of the last cosine in it is 100 FP32_PRE_MAX and more, so a plan capped one bin lower fails"""
    for name in EC.PROBE_ALONE:
        r = EC.row(name)
        for axis in (0, 1):
            N, M, origin, span = EC.axes(r)[axis]
            k = EC.last_kept(r, axis)
            assert k == N - 1
            y = _probe_outputs(r, axis, k)
            t = V.positions(M, origin, span)
            want = 0.5 + EC.PROBE_AMPLITUDE * np.cos(np.pi * k * (2 * t + 1) / (2 * N))
            line = y[0, 0, :] if axis == 0 else y[0, :, 0]
            # (the probe is the fp32 rounding of the basis vector: 2^-24 of its values)
            assert np.abs(line - want).max() <= 5e-7
            assert np.abs(want - 0.5).max() >= 100 * P.FP32_PRE_MAX
    a, b = EC.row("mirror_cap"), EC.row("mirror_cap_hi")
    x = np.random.default_rng(3).random((3, a[2], a[1]))
    # one ulp of the span moves the last position by 1e-14 pixels
    assert np.abs(EC.oracle_y(a, x) - EC.oracle_y(b, x)).max() <= 1e-11


def test_kmax_zero_is_the_mean():
    """k0, k0_m: every output row is constant, and its input row's mean once the shift along y is taken out (mean_view); k0_y the
    same for the columns.  And why the rows carry that shift: without it, on binary16 input, R = y / sc is a sum of eight binary16
    numbers and a good share of the values are exact ties between two binary16 numbers; with it none is"""
    for name, axis in EC.K0_ROWS:
        r = EC.row(name)
        x = np.random.default_rng(11).random((3, r[2], r[1]))
        y = EC.oracle_y(r, x)
        assert y.shape == (3, r[4], r[3]) and np.ptp(y, axis=axis).max() <= 1e-12, name
        ym = EC.oracle_y(EC.mean_view(r, axis), x)
        assert np.abs(ym - np.broadcast_to(x.mean(axis=axis, keepdims=True), ym.shape)).max() <= 1e-12, name

        def ties(row):
            xh = P.inputs(r[1], r[2], 2, False, 900 + r[1] + r[2])[2]
            Rr = EC.oracle_y(row, xh) / EC.scale(row)
            ulp = 2.0 ** (np.floor(np.log2(np.abs(Rr))) - 10)
            return int((np.abs((Rr / ulp) % 1 - 0.5) < 1e-6).sum())
        print("MEASURED %s: exact binary16 ties of R on binary16 input, without the shift %d, with it %d (of %d)" % (name, ties(EC.mean_view(r, axis)), ties(r), y.size))
        assert ties(r) == 0 and ties(EC.mean_view(r, axis)) >= 10
