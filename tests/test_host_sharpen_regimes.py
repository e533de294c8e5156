"""CPU: the table and the bars of tests/sharpen_regime_cases.py, proven with the oracle alone -- every row meets the conditions its
marks claim and no other, every pole fails them, the "%f" text of the strengths, flat planes, and each comparison raising on a single
value moved by twice its bar.  The plan's own text rounding of coef and upsq (plan_rules.cpp) against the oracle's, through the
device-free plan driver."""
import numpy as np
import pytest

import oraclelib as O
import plan_driver
import sharpen_regime_cases as S

SHAPES = ((28, 12, 1.5), (256, 24, 2.0))          # the stand-alone kernels' shapes: k_sharpen, k_sharpen_t


@pytest.fixture(scope="module")
def held():
    """{(regime, strength): [conditions() per shape]} for every pair of the grid, poles included"""
    return {(r, s): [S.conditions(W, H, u, r, s, K=2) for (W, H, u) in SHAPES] for r in S.REGIMES for s in S.STRENGTHS}


def test_the_table_is_the_grid_without_the_poles():
    listed = [(r, s) for (r, s, _) in S.CASES]
    assert len(set(listed)) == len(listed)
    assert set(listed) == {(r, s) for r in S.REGIMES for s in S.STRENGTHS} - set(S.POLES)
    assert all((r in S.REGIMES and s in S.STRENGTHS) for (r, s) in S.POLES) and len(set(S.POLES)) == 7
    assert all(set(m.split()) <= {"iso", "e2e", "p2"} and m.split() for (_, _, m) in S.CASES)
    for mark in ("iso", "e2e", "p2"):
        assert S.rows(mark)


def test_every_row_meets_exactly_the_conditions_it_is_marked_with(held):
    for (r, s, marks) in S.CASES:
        for mark in ("iso", "e2e", "p2"):
            holds = all(res[mark][1] for res in held[(r, s)])
            assert holds == (mark in marks.split()), (r, s, mark, [res[mark] for res in held[(r, s)]])


def test_every_pole_fails_the_conditions(held):
    for (r, s) in S.POLES:
        small, large = held[(r, s)]
        assert not any(large[m][1] for m in ("iso", "e2e", "p2")), (r, s, large)
        assert not (small["e2e"][1] or small["p2"][1]), (r, s, small)       # (on 42x18 pixels the pole can miss the isolation probe)


def test_ceilings_and_constants_are_the_projects_existing_bars():
    assert (S.ISO_CEILING, S.E2E_CEILING, S.P2_CEILING, S.NATIVE_RCP_FRAC) == (1e-4, 5e-4, 1.6e-2, 5e-3)
    assert S.EPS == {0: 2.0 ** -23, 1: 2.0 ** -52}
    # flat 0.5 at 0.24: fit for the isolation bar, too ill-conditioned for the other two
    res = S.conditions(256, 24, 2.0, "mid_flat", 0.24, K=2)
    assert res["iso"][1] and 4e-5 < res["iso"][0] < 6e-5
    assert not res["e2e"][1] and 5e-4 < res["e2e"][0] < 2e-3
    assert not res["p2"][1] and res["p2"][0] > 1.6e-2


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_strengths_reach_the_filter_as_six_decimal_text(precision):
    x = S.regime_planes(28, 12, "mid_wide", precision)
    R, out0 = S.oracle_R(x, 1.5, precision, 0.0)
    assert np.array_equal(S.oracle_R(x, 1.5, precision, 4e-7)[1], out0)                 # "0.000000"
    a, b = S.oracle_R(x, 1.5, precision, 0.1234567)[1], S.oracle_R(x, 1.5, precision, 0.123457)[1]
    assert np.array_equal(a, b)
    # (the seventh decimal is what is lost: the sixth still counts -- in binary16 both texts are the same constant)
    assert precision == 2 or not np.array_equal(a, S.oracle_R(x, 1.5, precision, 0.123456)[1])
    assert S.const_text(4e-7, precision) == 0.0 and S.const_text(0.1234567, precision) == S.const_text(0.123457, precision)
    for s in S.STRENGTHS:           # const_text is the oracle's constant: idempotent, and the same filter
        t = S.const_text(s, precision)
        assert S.const_text(t, precision) == t or precision == 2
        if precision != 2:
            assert np.array_equal(O.sharpen(R, 1.5, precision, t), O.sharpen(R, 1.5, precision, s))


def test_flat_planes_come_back_clamped():
    for tone in (0.0, 0.1, 0.5, 1.0, 1.3, -0.3):
        R = np.full((3, 6, 10), tone / 4.0)
        want = min(abs(tone), 1.0)
        for s in S.STRENGTHS:
            out = O.sharpen(R, 2.0, 0, s)
            assert np.abs(out - want).max() <= 1e-12, (tone, s)
    R16 = np.full((3, 6, 10), 0.25)
    for s in S.STRENGTHS:
        assert np.array_equal(O.sharpen(R16, 2.0, 2, s), np.ones_like(R16))             # (white: scale = 0, every operation exact)
        assert np.array_equal(O.sharpen(0.0 * R16, 2.0, 2, s), 0.0 * R16)


def _moved(out, bar):
    bad = out.copy()
    bad[1, out.shape[1] // 2, out.shape[2] // 3] += 2.0 * bar
    return bad


def test_each_comparison_raises_on_one_value_moved_by_twice_its_bar():
    u, s = 2.0, 0.5
    R, out = S.oracle_R(S.regime_planes(64, 16, "mid_wide", 0), u, 0, s)
    _, bar = S.assert_iso("host iso", out, R, u, 0, s)
    assert bar > 0
    with pytest.raises(AssertionError):
        S.assert_iso("host iso moved", _moved(out, bar), R, u, 0, s)
    _, bar = S.assert_e2e("host e2e", out, out, R, u, 0, s)
    assert bar >= 2e-5
    with pytest.raises(AssertionError):
        S.assert_e2e("host e2e moved", _moved(out, bar), out, R, u, 0, s)
    R1, out1 = S.oracle_R(S.regime_planes(64, 16, "mid_wide", 1), u, 1, s)
    _, bar1 = S.assert_e2e("host e2e p1", out1, out1, R1, u, 1, s)
    assert 1e-9 <= bar1 < bar
    with pytest.raises(AssertionError):
        S.assert_e2e("host e2e p1 moved", _moved(out1, bar1), out1, R1, u, 1, s)
    R16, out16 = S.oracle_R(S.regime_planes(64, 16, "mid_wide", 2), u, 2, s)
    _, bar16 = S.assert_p2("host p2", out16, out16, R16, u, s)
    assert bar16 > 0
    with pytest.raises(AssertionError):
        S.assert_p2("host p2 moved", _moved(out16, bar16), out16, R16, u, s)
    # ... and on too many values moved by one ulp of theirs (the share bar)
    many = S.half_step(out16, np.where(np.random.RandomState(3).rand(*out16.shape) < S.f_ref(R16, u, s) + 3.0 * S.NATIVE_RCP_FRAC, 1.0, 0.0))
    assert np.abs(many - out16).max() <= bar16
    with pytest.raises(AssertionError):
        S.assert_p2("host p2 share", many, out16, R16, u, s)
    # a bar above its ceiling, or an oracle output that is not finite, is refused whatever the kernel gives
    Rp, outp = S.oracle_R(S.regime_planes(256, 24, "high", 0), u, 0, 0.5)
    with pytest.raises(AssertionError):
        S.assert_iso("host iso pole", outp, Rp, u, 0, 0.5)
    with pytest.raises(AssertionError):
        S.assert_e2e("host e2e pole", outp, outp, Rp, u, 0, 0.5)


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_complex_image_filter_and_its_probes(precision):
    """oraclelib.sharpen_complex is the sharpen pass of the non-R2C pipeline; on a real image it is the real filter in fp32 / fp64
    (|t| against sqrt(t t)); the bars of a complex image move both of its parts"""
    x = S.regime_planes(48, 8, "black_signs", precision).astype(np.float64)
    z, out, _ = O.upscale_planes_complex(x, 2.0, precision, 0.5)
    assert np.abs(z.imag).max() > 0
    assert np.array_equal(O.sharpen_complex(z, 2.0, precision, 0.5), out)
    if precision != 2:
        assert np.abs(O.sharpen_complex(z.real + 0j, 2.0, precision, 0.5) - O.sharpen(z.real, 2.0, precision, 0.5)).max() <= 1e-12
        bar = S.t_e2e(z, 2.0, precision, 0.5, base=out)
        assert bar <= S.E2E_CEILING
        with pytest.raises(AssertionError):
            S.assert_e2e("host complex e2e moved", _moved(out, bar), out, None, 2.0, precision, 0.5, bar=bar)
    else:
        bar, share = S.t16(z, 2.0, 0.0), S.f_ref(z, 2.0, 0.0)
        assert 0.0 < bar <= S.P2_CEILING and 0.0 < share < 0.05
        # a part so small that its binary16 square is 0 or one subnormal step (t = 724 2^-22: t t = 0.4999 2^-24, and 0.5013 2^-24 one
        # ulp of z higher): a one-ulp move of the part moves the tap from 0 to sqrt(2^-24) = 2^-12, which a probe on the modulus
        # image does not see
        tiny = np.full((3, 4, 6), 724.0 * 2.0 ** -24) + 0j
        assert S.t16(tiny, 2.0, 0.0) >= 2.0 ** -12 > 8.0 * S.t16(np.abs(tiny), 2.0, 0.0)
        moved = S.half_step(z, np.ones(z.shape) + 1j * np.ones(z.shape))
        assert (moved.real > z.real).all() and (moved.imag > z.imag).all()


def test_half_step_moves_every_value_one_binary16_ulp():
    h = np.array([0.0, 1.0, 0.25, -0.5, 6.1e-5, 2.0 ** -24]).astype(np.float16).astype(np.float64)
    up, dn = S.half_step(h, np.ones_like(h)), S.half_step(h, -np.ones_like(h))
    assert np.array_equal(S.half_step(h, np.zeros_like(h)), h)
    assert (up > h).all() and (dn < h).all()
    assert up[1] == 1.0 + 2.0 ** -10 and dn[1] == 1.0 - 2.0 ** -11 and up[0] == 2.0 ** -24 and dn[5] == 0.0


def test_planes_are_tone_plus_amp_times_a_periodic_texture():
    t = S.tex(96, 48, 5)
    assert t.shape == (3, 48, 96) and np.allclose(np.abs(t).max(axis=(1, 2)), 1.0)
    assert not np.allclose(t[0], t[1]) and not np.allclose(t[1], t[2])               # each channel shifted differently
    for (tone, amp) in S.REGIMES.values():
        p = S.planes(96, 48, tone, amp, 5, 1)
        assert np.allclose(p, tone + amp * t) and p.dtype == np.float64
    assert S.planes(8, 4, 0.5, 0.2, 0, 2).dtype == np.float16 and S.planes(8, 4, 0.5, 0.2, 0).dtype == np.float32
    codes = S.regime_codes(16, 8, "mid_wide")
    assert codes.shape == (8, 16, 3) and codes.dtype == np.uint8
    # regimes of their kind: values clamped, negative, crossing zero, both branches
    assert (S.regime_planes(64, 32, "all_clamped") >= 1.0).all() and (S.regime_planes(64, 32, "negative") < 0).all()
    z = S.regime_planes(64, 32, "zero_crossing")
    assert (z < 0).any() and (z > 0).any()
    w = S.regime_planes(64, 32, "white_half_clamped")
    assert 0.2 < (w > 1.0).mean() < 0.8
    assert S.regime_planes(64, 32, "dark").max() < 0.5 < S.regime_planes(64, 32, "bright").min()


def test_smallest_sizes_of_the_paths_found_without_a_device():
    """the smallest -p 1 width of the non-R2C path, and the smallest -u 2 / -u 1.5 sizes with kernels specialised at plan time
    (fftup_jit_check with arch "": the chooser alone, nothing is compiled)"""
    import ctypes as C
    from vkresample_amd import _lib
    assert next(W for W in range(2, 4096, 2) if O.check(W, 4, 2.0, 1) == 0 and O.uses_complex_path(W, 4, 2.0, 1)) == S.CPLX_P1_W
    lib, buf = _lib.load(), C.create_string_buffer(256)
    sizes = sorted((W * H, W, H) for W in range(2, 130, 2) for H in range(2, 130, 2))
    for u, want in S.JIT_SMALLEST.items():
        got = next((W, H) for (_, W, H) in sizes if all(lib.fftup_jit_check(W, H, u, p, b"", buf, 256) == 0 for p in (0, 2)))
        assert got == want and O.check(got[0], got[1], u, 0) == 0, (u, got)


def test_plan_constants_match_the_oracles_text_rounding(tmp_path):
    """coef and upsq as plan_rules.cpp rounds them ("%f" text, then the arithmetic's type) for every listed strength"""
    reqs, want = [], []
    for (W, H, u) in SHAPES + ((512, 256, 2.0),):
        for precision in (0, 2):
            for s in S.STRENGTHS + (0.2, 0.123457):
                reqs.append(plan_driver.request_line("create", W, H, u, precision, 0, sharpen=s))
                want.append((S.const_text(u * u, precision), S.const_text(s, precision)))
    got = plan_driver.run(plan_driver.build(tmp_path), tmp_path, reqs)
    for line, (upsq, coef), rq in zip(got, want, reqs):
        assert not line.startswith("error"), (rq, line)
        g = plan_driver.fields(line)
        assert float.fromhex(g["upsq"]) == upsq and float.fromhex(g["coef"]) == coef, (rq, g["upsq"], g["coef"], upsq, coef)
