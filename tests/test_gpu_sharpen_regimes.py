"""GPU: every sharpen kernel against the oracle across strengths and tone regimes (tests/sharpen_regime_cases.py: the frames, the
literal case table and the bars, all derived from the oracle alone and proven on the CPU by tests/test_host_sharpen_regimes.py).

One parametrised test per kernel, at the smallest shape that crosses the kernel's seams; each asserts what the plan says about the
kernels it runs (kernel_names, tuned, description) beside the sizes that select the sharpen kernel (csrc/fftup_launch.hip:
fast_sharpen_ok, uW a multiple of 256 and uH of 16 -> k_sharpen_t, k_sharpen otherwise).  Every comparison prints its figures next
to its bar (MEASURED lines under pytest -s: profiles/sharpen_regimes_measured.txt)."""
import functools

import numpy as np
import pytest

import oraclelib as O
import sharpen_regime_cases as S
import view_oracle as V
from paritylib import measured

pytestmark = pytest.mark.gpu

ISO = S.rows("iso")
E2E = S.rows("e2e")
P2 = S.rows("p2")
IDS = lambda rows: [S.case_id(r, s) for (r, s) in rows]       # noqa: E731

# the fused kernels: both branches of the quotient, the flats, both clamps, the tie; s in {0, 0.5, 1.0, -0.2}
FUSED = (("dark", 0.5), ("bright", 0.5), ("black_flat", 1.0), ("white_flat", 1.0), ("white_half_clamped", -0.2), ("all_clamped", 0.0),
         ("mid_wide", 1.0), ("mid_flat", 0.5))
assert set(FUSED) <= set(E2E) & set(P2) and len(FUSED) <= 8
K_FUSED = 2             # probes per case on the larger frames (the fused kernels, the non-R2C path)


def _v():
    import vkresample_amd as v
    return v


def _run(up, x=None, rgb=None, pre=True):
    if rgb is not None:
        up.upload_rgb8(rgb)
    else:
        up.upload_planar(x)
    up.execute(1)
    return (up.download_presharpen().astype(np.float64) if pre else None), up.download_planar().astype(np.float64)


def _unfused_generic(up, fast, double=False):
    """an unfused plan of the size-generic kernels, and the sharpen kernel its sizes select"""
    assert up.kernel_names == ["row_r2c", "col_fwd_pad_inv", "row_c2r", "sharpen"] and up.num_kernels == 4 and not up.tuned, (up.kernel_names, up.tuned)
    assert up.description.startswith("size-generic kernels") and ("double" in up.description) == double, up.description
    assert (up.out_width % 256 == 0 and up.out_height % 16 == 0 and not double) == fast, (up.out_width, up.out_height)


def _alone(tag, W, H, u, regime, s, precision, flags, fast, out_size):
    """a stand-alone sharpen kernel on the device's own pre-sharpen planes: T_iso in fp32 / fp64, bit for bit in binary16"""
    x = S.regime_planes(W, H, regime, precision)
    with _v().Upscaler(W, H, u, precision, s, 0, flags) as up:
        _unfused_generic(up, fast, double=precision == 1)
        assert (up.out_width, up.out_height) == out_size
        pre, out = _run(up, x)
    name = "%s %s p%d" % (tag, S.case_id(regime, s), precision)
    if precision == 2:
        want = O.sharpen(pre, u, 2, s)
        measured(name, differing=float((out != want).sum()), values=out.size)
        assert np.isfinite(want).all() and np.array_equal(out, want)
    else:
        S.assert_iso(name, out, pre, u, precision, s)


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("regime,s", ISO, ids=IDS(ISO))
def test_k_sharpen(regime, s, precision):
    """k_sharpen<false|true>: 28x12 -u 1.5 -> 42x18 (a scalar tail of two pixels, rows of one workgroup)"""
    v = _v()
    _alone("k_sharpen", 28, 12, 1.5, regime, s, precision, v.FLAG_UNFUSED_SHARPEN | v.FLAG_GENERIC_KERNELS, False, (42, 18))


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("regime,s", ISO, ids=IDS(ISO))
def test_k_sharpen_t(regime, s, precision):
    """k_sharpen_t<false|true>: 256x24 -u 2 -> 512x48 (two x blocks, three y blocks)"""
    _alone("k_sharpen_t", 256, 24, 2.0, regime, s, precision, _v().FLAG_UNFUSED_SHARPEN, True, (512, 48))


@pytest.mark.parametrize("regime,s", ISO, ids=IDS(ISO))
def test_k_sharpen_f64(regime, s):
    """k_sharpen_f64<true>: 320x20 -u 2 -p 1 -> 640x40 (two x blocks of 512, 16-row blocks with a ragged tail of 8).  The odd-width
    instantiation k_sharpen_f64<false> has no plan: -p 1 exists for even output sizes only (odd sizes: -p 0 and -p 2)."""
    _alone("k_sharpen_f64", 320, 20, 2.0, regime, s, 1, 0, False, (640, 40))


# ---------------------------------------------------------------------------------------------------- the non-R2C path: k_sharpen_c
CPLX_P1_W = S.CPLX_P1_W   # the smallest -p 1 width on the non-R2C path (tests/test_host_sharpen_regimes.py)


@functools.lru_cache(maxsize=None)
def _cplx_oracle(W, regime, s, precision):
    """(the oracle's complex pre-sharpen image, its output, the bars).  The filter's taps are |u^2 z|: the probes move both parts of z
    and run the oracle's filter of the complex image (oraclelib.sharpen_complex) -- in binary16 the squares of small parts fall on
    the subnormal grid, and a one-ulp move of a part near zero moves a tap by sqrt(2^-24) = 2.4e-4."""
    x = S.regime_planes(W, 4, regime, precision).astype(np.float64)
    z, out, _ = O.upscale_planes_complex(x, 2.0, precision, s)
    if precision == 2:
        return z, out, (S.t16(z, 2.0, s, K_FUSED, base=out), S.f_ref(z, 2.0, s, base=out))
    return z, out, S.t_e2e(z, 2.0, precision, s, K_FUSED, base=out)


def _cplx(W, regime, s, precision):
    v = _v()
    assert O.uses_complex_path(W, 4, 2.0, precision)
    z, want, bars = _cplx_oracle(W, regime, s, precision)
    with v.Upscaler(W, 4, 2.0, precision, s) as up:
        assert up.kernel_names[0] == "row_c2c" and up.kernel_names[2:] == ["row_c2c_inv", "sharpen"] and not up.tuned, up.kernel_names
        assert "non-R2C path" in up.description, up.description
        _, out = _run(up, S.regime_planes(W, 4, regime, precision), pre=False)
    name = "k_sharpen_c %dx4 %s p%d" % (W, S.case_id(regime, s), precision)
    if precision == 2:
        S.assert_p2(name, out, want, None, 2.0, s, bars=bars)
    else:
        S.assert_e2e(name, out, want, None, 2.0, precision, s, bar=bars)


@pytest.mark.parametrize("regime,s", E2E, ids=IDS(E2E))
def test_k_sharpen_c_fp32(regime, s):
    """k_sharpen_c<float2>: 4608x4 -u 2 (uW = 9216 > 8192: 36 workgroups per row)"""
    _cplx(4608, regime, s, 0)


@pytest.mark.parametrize("regime,s", P2, ids=IDS(P2))
def test_k_sharpen_c_fp16(regime, s):
    """k_sharpen_c<float2, true>: the complex modulus in binary16 arithmetic"""
    _cplx(4608, regime, s, 2)


@pytest.mark.parametrize("regime,s", E2E, ids=IDS(E2E))
def test_k_sharpen_c_fp64(regime, s):
    """k_sharpen_c<double2>: the smallest -p 1 width of the non-R2C path"""
    _cplx(CPLX_P1_W, regime, s, 1)


# ------------------------------------------------------------------------------------------------------------- the fused kernels
@functools.lru_cache(maxsize=None)
def _oracle(W, H, u, regime, s, precision):
    """(R, out, bars) of the oracle's own pipeline: T_e2e in fp32, (T16, f_ref) in binary16"""
    R, out = S.oracle_R(S.regime_planes(W, H, regime, precision), u, precision, s)
    if precision == 2:
        return R, out, (S.t16(R, u, s, K_FUSED, base=out), S.f_ref(R, u, s, base=out))
    return R, out, S.t_e2e(R, u, precision, s, K_FUSED, base=out)


def _fused_against_unfused_and_oracle(tag, W, H, u, regime, s, precision, check_fused, check_unfused):
    v = _v()
    x = S.regime_planes(W, H, regime, precision)
    R, want, bars = _oracle(W, H, u, regime, s, precision)
    with v.Upscaler(W, H, u, precision, s) as up:
        assert up.kernel_names[2:] == ["row_c2r_sharpen", "-"] and up.num_kernels == 3, up.kernel_names
        check_fused(up)
        _, fused = _run(up, x, pre=False)
    with v.Upscaler(W, H, u, precision, s, 0, v.FLAG_UNFUSED_SHARPEN) as up:
        assert up.kernel_names[2:] == ["row_c2r", "sharpen"] and up.num_kernels == 4, up.kernel_names
        check_unfused(up)
        _, unfused = _run(up, x, pre=False)
    name = "%s %dx%d u%g %s p%d" % (tag, W, H, u, S.case_id(regime, s), precision)
    # (the deferred pixel, column uW - 1, once more on its own: its taps wrap into the next row and it is evaluated apart)
    for what, got, ref in (("vs unfused", fused, unfused), ("vs oracle", fused, want), ("last column vs unfused", fused[:, :, -1:], unfused[:, :, -1:]),
                           ("last column vs oracle", fused[:, :, -1:], want[:, :, -1:]), ("unfused vs oracle", unfused, want)):
        if precision == 2:
            if what.startswith("last column"):       # (a share of 1 / uW of the values: the magnitude alone)
                err = float(np.abs(got - ref).max())
                measured("%s %s" % (name, what), p2_max=err, T16=bars[0])
                assert err <= bars[0]
            else:
                S.assert_p2("%s %s" % (name, what), got, ref, R, u, s, bars=bars)
        else:
            S.assert_e2e("%s %s" % (name, what), got, ref, R, u, precision, s, bar=bars)


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("regime,s", FUSED, ids=IDS(FUSED))
def test_fused_ahead_of_time(regime, s, precision):
    """the fused C2R+sharpen kernel of the power-of-two plans (packed fp32 / packed binary16 evaluators, deferred pixel): 512x256 -u 2"""
    def fused(up):
        assert up.tuned and not up.specialised_at_plan_time and "ahead-of-time power-of-two kernels" in up.description and "fused C2R+sharpen on" in up.description, up.description

    def unfused(up):
        assert up.tuned and "fused C2R+sharpen off" in up.description, up.description
    _fused_against_unfused_and_oracle("fused_aot", 512, 256, 2.0, regime, s, precision, fused, unfused)


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("u", [2.0, 1.5])
@pytest.mark.parametrize("regime,s", FUSED, ids=IDS(FUSED))
def test_fused_plan_time(regime, s, u, precision):
    """the fused kernel instantiated at plan time, at the smallest -u 2 and -u 1.5 sizes that have one (found without a device:
    tests/test_host_sharpen_regimes.py)"""
    W, H = S.JIT_SMALLEST[u]

    def fused(up):
        assert up.specialised_at_plan_time and up.description.startswith("specialised at plan time") and "fused" in up.description, up.description

    def unfused(up):
        assert not up.tuned and up.description.startswith("size-generic kernels"), up.description
    _fused_against_unfused_and_oracle("fused_jit", W, H, u, regime, s, precision, fused, unfused)


U8_CASES = (("mid_wide", 0.24), ("bright", 0.5))


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("wrap", [0, 1])
@pytest.mark.parametrize("regime,s", U8_CASES, ids=IDS(U8_CASES))
def test_fused_u8_store(regime, s, wrap, precision):
    """the OUT_U8 stores of the fused kernel against the conversion launch on the planes of the same plan without the flag, under the
    sweep's rule (tests/test_gpu_sweep.py): at most one code apart, at most max(3, 1e-5 n) values differing (1e-4 n at -p 2).  Under
    FFTUP_FLAG_U8_WRAP the codes are residues modulo 256, and so is their distance.  (On these band-limited frames the oracle's
    outputs stay inside [0, 1]: 0.178 .. 0.796 and 0.900 .. 0.993.  The filter limits itself at black and white -- n -> 0 there --
    and leaves the range only beside a pole, which no case may be: the saturating and wrapping ends of the conversion stay with
    tests/test_gpu_parity.py::test_u8_wrap_flag.)"""
    v = _v()
    rgb = S.regime_codes(512, 256, regime)
    flags = v.FLAG_U8_WRAP if wrap else 0
    with v.Upscaler(512, 256, 2.0, precision, s, 0, flags) as up:
        assert not up.u8_store and up.kernel_names[2] == "row_c2r_sharpen" and up.tuned
        _, planes = _run(up, rgb=rgb, pre=False)
        ref = up.download_rgb8()
    with v.Upscaler(512, 256, 2.0, precision, s, 0, flags | v.FLAG_FUSE_U8_STORE) as up:
        assert up.u8_store and "8-bit RGB store" in up.description and up.kernel_names[2] == "row_c2r_sharpen" and up.tuned, up.description
        up.upload_rgb8(rgb)
        up.execute(1)
        got = up.download_rgb8()
    d = np.abs(got.astype(int) - ref.astype(int))
    if wrap:
        d = np.minimum(d, 256 - d)
    measured("fused_u8 %s wrap%d p%d" % (S.case_id(regime, s), wrap, precision), max_codes=d.max(), differing=(d != 0).sum(),
             allowed=max(3, (1e-5 if precision == 0 else 1e-4) * d.size), below0=(planes < 0).mean(), above1=(planes > 1).mean())
    assert np.isfinite(planes).all()
    assert d.max() <= 1
    assert (d != 0).sum() <= max(3, (1e-5 if precision == 0 else 1e-4) * d.size)


# ------------------------------------------------------------------------------------------------------------------ a family plan
VIEW = (40, 24, 66, 40, (2.25, 1.5), (36.0, 22.0))       # u_e^2 = 66 * 40 / (36 * 22) = 3.33333..: text "3.333333"


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("regime,s", ISO, ids=IDS(ISO))
def test_view_plan_sharpen(regime, s, precision):
    """a view plan, whose factor is no six-decimal number: k_sharpen with upsq = "%f"(u_e u_e) against oraclelib.sharpen(.., u_e, ..)"""
    W, H, uW, uH, origin, span = VIEW
    u_e = V.effective_factor(uW, uH, span)
    assert "%f" % float(np.float32(u_e) * np.float32(u_e)) == "3.333333"
    x = S.regime_planes(W, H, regime, precision)
    with _v().Upscaler.view(W, H, uW, uH, origin, span, precision, s) as up:
        assert up.kernel_names[2:] == ["row_view_c2r", "sharpen"] and up.description.startswith("view:"), (up.kernel_names, up.description)
        pre, out = _run(up, x)
    name = "view_sharpen %s p%d" % (S.case_id(regime, s), precision)
    if precision == 2:
        want = O.sharpen(pre, u_e, 2, s)
        measured(name, differing=float((out != want).sum()), values=out.size)
        assert np.isfinite(want).all() and np.array_equal(out, want)
    else:
        S.assert_iso(name, out, pre, u_e, 0, s)
