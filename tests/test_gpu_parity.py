"""GPU parity: HIP path (through the C ABI) vs the CPU oracle on the same seeded inputs.

Tolerances (north_star: "within 1e-4 rel-err"); every bound is about ten times the largest figure any parametrisation of the
test measured (printed as MEASURED / PARITY lines under pytest -s: profiles/r04_h_parity_small.txt), so it is the error budget
of THIS code and not of the task:
  fp32 (-p 0): pre-sharpen image t = u^2*g: relative L2 error <= 2e-6 (measured <= 2.2e-7), max |err| <= 1e-5 of full scale
      (<= 9.5e-7).  Sharpened output, natural-like frames: relative L2 <= 5e-6, max |err| <= 2e-5 (4.4e-7 / 1.7e-6).
      Uniform-noise frames: max |err| <= 5e-4 (4.4e-5) -- the reference's filter has scale = -s*sqrt(min(a,b)), whose slope is
      unbounded at 0, so an fp32 rounding error of 1e-7 in a neighbourhood minimum that is exactly 0 in fp64 becomes ~1e-4 in the
      output (black / white pixels of the uniform-random frames hit this; with -u 1, where every pixel keeps its exact 0 or
      1, 2.5e-4 measured, 2.5e-3 allowed).  The sharpen kernel itself is checked against the oracle's sharpen applied to the
      *device's own* pre-sharpen planes: <= 3e-6 natural (2.8e-7), <= 1e-4 uniform (1.1e-5).
  fp16 (-p 2): the path stores fp16 (half ulp 2.4e-4 at 0.5), so: pre-sharpen within 1 half-ulp of the oracle's own fp16 value
      and different from it in <= 1 % of the pixels (0.1 %), sharpened output relative L2 <= 3.5e-4 (3.5e-5), different from the
      oracle in <= 2 % of the pixels (0.18 %), max |err| <= 8e-3 = 16 ulps (6 measured: errors come in whole ulps, a one-ulp
      flip of an fp16 input moves the fp16-arithmetic filter by a few).
The last output row is compared like every other: the reference reads stale padding memory there (quirk B5), this project
defines those reads as "same column, last written row" (oracle/fftup_oracle.c) and every comparison holds the HIP path to that
definition.  tests/test_gpu_last_row.py aims at the row itself.
"""
import os

import numpy as np
import pytest

import oraclelib as O
from paritylib import measured, one_half_ulp_bound, rel_l2, within_one_half_ulp

pytestmark = pytest.mark.gpu


def _up(*a, **k):
    import vkresample_amd as v
    return v.Upscaler(*a, **k)


def _run(W, H, u, precision, dist, flags=0, sharpen=0.2, seed=0):
    from vkresample_amd import synth
    rgb = synth.frame(seed, W, H, dist)
    with _up(W, H, u, precision, sharpen, 0, flags) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        pre = up.download_presharpen().astype(np.float64)
        out = up.download_planar().astype(np.float64)
        u8 = up.download_rgb8()
    opre, oout, ou8 = O.upscale_rgb8(rgb, u, precision, sharpen)
    return (pre, out, u8), (opre, oout, ou8)


SIZES_FP32 = [
    (16, 8, 2.0), (20, 12, 2.0), (64, 32, 2.0), (60, 42, 2.0),      # 60=4*3*5, 42=2*3*7
    (16, 8, 1.5), (32, 16, 1.0), (24, 16, 3.0), (256, 128, 2.0), (240, 270, 2.0),
    (512, 256, 2.0), (1024, 512, 2.0),                              # size-specialised kernels
]


@pytest.mark.parametrize("W,H,u", SIZES_FP32)
@pytest.mark.parametrize("dist", ["U", "N"])
def test_fp32_parity_small(W, H, u, dist):
    (pre, out, u8), (opre, oout, ou8) = _run(W, H, u, 0, dist)
    usq = u * u
    measured("fp32_small %dx%d u%g %s" % (W, H, u, dist), pre_l2=rel_l2(pre, opre), pre_max=np.abs(pre - opre).max() * usq,
             out_l2=rel_l2(out, oout), out_max=np.abs(out - oout).max())
    assert rel_l2(pre, opre) <= 2e-6
    assert np.abs(pre - opre).max() * usq <= 1e-5
    # (uniform noise: the filter's sqrt at exact zeros, see the module docstring; -u 1 keeps every exact 0 and 1)
    l2_max, out_max = (5e-6, 2e-5) if dist == "N" else ((3e-4, 2.5e-3) if u == 1.0 else (5e-6, 5e-4))
    assert rel_l2(out, oout) <= l2_max
    assert np.abs(out - oout).max() <= out_max
    # sharpen kernel in isolation: same (device) input on both sides (two-launch path, where the
    # pre-sharpen planes are exactly what the sharpen kernel read)
    from vkresample_amd import FLAG_UNFUSED_SHARPEN
    (pre_u, out_u, _), _ = _run(W, H, u, 0, dist, flags=FLAG_UNFUSED_SHARPEN)
    sh = O.sharpen(pre_u, u, 0, 0.2)
    measured("fp32_small sharpen alone %dx%d u%g %s" % (W, H, u, dist), max=np.abs(out_u - sh).max())
    # uniform noise: n = 1 - mx cancels in fp32 for near-saturated neighbourhoods (as in the reference's fp32 shader)
    assert np.abs(out_u - sh).max() <= (3e-6 if dist == "N" else 1e-4)
    # u8 = trunc(255*x): a float error can flip the truncation by one code; for u == 1 every exact
    # output sits ON a code boundary (x = k/255), so only the magnitude is asserted there
    d = np.abs(u8.astype(int) - ou8.astype(int))
    assert d.max() <= 1
    if u != 1.0:
        assert (d != 0).mean() <= 5e-3


@pytest.mark.parametrize("W,H,u", [(64, 32, 2.0), (60, 42, 2.0), (256, 128, 2.0), (512, 256, 2.0)])
def test_fp32_fused_u8_load_identical(W, H, u):
    from vkresample_amd import FLAG_FUSE_U8_LOAD
    (pre, out, u8), _ = _run(W, H, u, 0, "U")
    (pre2, out2, u82), _ = _run(W, H, u, 0, "U", flags=FLAG_FUSE_U8_LOAD)
    assert np.array_equal(pre, pre2) and np.array_equal(out, out2) and np.array_equal(u8, u82)


@pytest.mark.parametrize("W,H,u", [(16, 8, 2.0), (64, 32, 2.0), (60, 42, 2.0), (256, 128, 2.0), (512, 256, 2.0)])
@pytest.mark.parametrize("dist", ["U", "N"])
def test_fp16_parity_small(W, H, u, dist):
    (pre, out, u8), (opre, oout, ou8) = _run(W, H, u, 2, dist)
    # pre-sharpen: both sides are fp16 values; fp32-vs-fp64 FFT noise can flip a rounding -> <= 1 ulp (paritylib)
    assert within_one_half_ulp(pre, opre).all()
    measured("fp16_small %dx%d u%g %s" % (W, H, u, dist), pre_diff_frac=(pre != opre).mean(), out_l2=rel_l2(out, oout),
             out_max=np.abs(out - oout).max(), out_diff_frac=(out != oout).mean())
    assert (pre != opre).mean() <= 0.01      # ringing around zero: fp16 ulp shrinks with |g|, fp32 noise does not
    assert rel_l2(out, oout) <= 3.5e-4 and (out != oout).mean() <= 0.02
    assert np.abs(out - oout).max() <= 8e-3
    # the half-arithmetic sharpen is bit-exact given the same fp16 input (two-launch path)
    from vkresample_amd import FLAG_UNFUSED_SHARPEN
    (pre_u, out_u, _), _ = _run(W, H, u, 2, dist, flags=FLAG_UNFUSED_SHARPEN)
    sh = O.sharpen(pre_u, u, 2, 0.2)
    assert np.array_equal(out_u, sh)


@pytest.mark.parametrize("precision", [0, 2])
def test_tuned_equals_generic(precision):
    """size-specialised kernels vs the size-generic ones on the same frame (fp32 rounding differences only)"""
    from vkresample_amd import FLAG_GENERIC_KERNELS
    (pre, out, u8), _ = _run(512, 256, 2.0, precision, "N")
    (pre2, out2, u82), _ = _run(512, 256, 2.0, precision, "N", flags=FLAG_GENERIC_KERNELS)
    measured("tuned_vs_generic p%d" % precision, pre_max=np.abs(pre - pre2).max() * 4, out_max=np.abs(out - out2).max(), out_diff_frac=(out != out2).mean())
    assert np.abs(pre - pre2).max() * 4 <= (4e-6 if precision == 0 else 1e-3)           # (measured 4.2e-7 / one binary16 ulp)
    assert np.abs(out - out2).max() <= (2e-5 if precision == 0 else 4e-3)              # (1.6e-6 / 2.4e-3 = five ulps)
    assert precision == 0 or (out != out2).mean() <= 2.5e-3                              # (2.2e-4)


def test_u8_conversion_bit_exact():
    """a1 (VR:1644 / VR:1676): the device conversion equals the reference expression for all 256 codes."""
    rgb = np.zeros((8, 64, 3), dtype=np.uint8)
    rgb[..., 0] = (np.arange(512) % 256).reshape(8, 64)
    rgb[..., 1] = 255 - rgb[..., 0]
    rgb[..., 2] = (rgb[..., 0].astype(int) * 7 % 256).astype(np.uint8)
    for precision in (0, 2):
        lut = O.load_lut(precision)
        with _up(64, 8, 2.0, precision) as up:
            up.upload_rgb8(rgb)
            got = up.download_input_planar().astype(np.float64)
        for c in range(3):
            assert np.array_equal(got[c], lut[rgb[..., c]])


def test_sharpen_fp16_bit_exact_given_same_R():
    """With identical fp16 R, the half-arithmetic sharpen must equal the oracle bit for bit.
    Constant and two-level images give an R that is exact in both implementations."""
    W, H = 32, 16
    rgb = np.zeros((H, W, 3), dtype=np.uint8)
    rgb[:, :, 0] = 255
    rgb[:, :, 1] = 51
    rgb[:, :, 2] = 0
    (pre, out, u8), (opre, oout, ou8) = _run_rgb(rgb, 2.0, 2)
    assert np.array_equal(pre, opre)
    assert np.array_equal(out, oout)


def _run_rgb(rgb, u, precision, sharpen=0.2, flags=0):
    H, W, _ = rgb.shape
    with _up(W, H, u, precision, sharpen, 0, flags) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        pre = up.download_presharpen().astype(np.float64)
        out = up.download_planar().astype(np.float64)
        u8 = up.download_rgb8()
    opre, oout, ou8 = O.upscale_rgb8(rgb, u, precision, sharpen)
    return (pre, out, u8), (opre, oout, ou8)


def test_kat_constant_exact():
    """KAT1: constant image -> same constant, sharpen included."""
    rgb = np.empty((16, 32, 3), dtype=np.uint8)
    rgb[..., 0], rgb[..., 1], rgb[..., 2] = 200, 17, 255
    (pre, out, u8), _ = _run_rgb(rgb, 2.0, 0)
    for c, v in enumerate((200, 17, 255)):
        x = np.float32(v) / np.float32(255)
        assert np.abs(out[c] - x).max() <= 2e-6
    assert np.abs(u8.astype(int) - rgb[0, 0].astype(int)).max() <= 1


def test_kat_cosine_planar_input():
    """KAT2/KAT3/KAT5 through the planar upload entry (analytic inputs)."""
    W, H, u = 64, 32, 2.0
    x = np.arange(W)[None, :]
    y = np.arange(H)[:, None]
    k0 = 5
    planes = np.stack([
        0.5 + 0.25 * np.cos(2 * np.pi * k0 * x / W) + 0 * y,            # KAT2
        0.5 + 0.1 * (-1.0) ** x + 0 * y,                                # KAT3: amplitude doubles
        0.5 + 0.1 * (-1.0) ** y * np.cos(2 * np.pi * 3 * x / W),        # KAT5
    ]).astype(np.float32)
    with _up(W, H, u, 0) as up:
        up.upload_planar(planes)
        up.execute(1)
        pre = up.download_presharpen().astype(np.float64) * (u * u)
    X = np.arange(int(u * W))[None, :]
    Y = np.arange(int(u * H))[:, None]
    exp0 = 0.5 + 0.25 * np.cos(2 * np.pi * k0 * X / (u * W)) + 0 * Y
    exp1 = 0.5 + 0.2 * np.cos(np.pi * X / u) + 0 * Y
    exp2 = 0.5 + 0.1 * np.cos(2 * np.pi * 3 * X / (u * W) - np.pi * Y / u)
    for got, exp in zip(pre, (exp0, exp1, exp2)):
        assert np.abs(got - exp).max() <= 5e-6


def test_error_codes():
    import vkresample_amd as v
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(2 * 11 * 64, 64)          # KAT8: non-smooth size
    assert e.value.code == 2
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(64, 64, precision=3)
    assert e.value.code == 3
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(63, 64)
    assert e.value.code == 1
    with _up(64, 32) as up:
        with pytest.raises(v.FftupError) as e:
            up.execute(1)                     # nothing uploaded
        assert e.value.code == 7


def test_repeat_is_deterministic_and_ring():
    from vkresample_amd import synth
    W, H = 128, 64
    with _up(W, H, 2.0, 0, ring=3) as up:
        frames = [synth.frame(k, W, H) for k in range(3)]
        for s, f in enumerate(frames):
            up.upload_rgb8(f, slot=s)
        up.execute_ring(6, 0)
        outs = [up.download_planar(s) for s in range(3)]
        up.execute_ring(3, 0)
        outs2 = [up.download_planar(s) for s in range(3)]
    for a, b in zip(outs, outs2):
        assert np.array_equal(a, b)
    assert not np.array_equal(outs[0], outs[1])
    for s, f in enumerate(frames):
        _, oout, _ = O.upscale_rgb8(f, 2.0, 0)
        assert np.abs(outs[s] - oout).max() <= 1e-3


def _report(tag, err, thr):
    """error distribution of a full-size comparison: printed (pytest -s / the committed profiles/*_parity.txt) and
    returned, so that the tail is a number and not a story"""
    a = np.abs(err).ravel()
    p50, p99, p9999 = np.percentile(a, [50, 99, 99.99])          # (one partition pass for the three)
    stats = {"p50": float(p50), "p99": float(p99), "p99.99": float(p9999),
             "max": float(a.max()), "count_above": int((a > thr).sum()), "n": int(a.size), "thr": thr}
    print("PARITY %s: p50 %.3g  p99 %.3g  p99.99 %.3g  max %.3g  count(>%g) %d of %d (%.2e)"
          % (tag, stats["p50"], stats["p99"], stats["p99.99"], stats["max"], thr, stats["count_above"], stats["n"],
             stats["count_above"] / stats["n"]))
    return stats


FULL_SIZE = [(2048, 1024, 0, 0), (2048, 1024, 0, 2), (1920, 1080, 0, 0), (1920, 1080, 0, 2), (2048, 1024, 2, 0), (2048, 1024, 2, 2),
             (1920, 1080, 2, 2), (1280, 720, 0, 0), (1280, 720, 0, 2), (1280, 720, 2, 0), (1280, 720, 2, 2)]


@pytest.mark.parametrize("W,H,precision,flags", FULL_SIZE)
@pytest.mark.parametrize("dist", ["N", "U"])
def test_full_size_vs_oracle(W, H, precision, flags, dist):
    """BASELINE configs 2-4 at full size against the (multi-threaded) oracle; flags = 2 is FFTUP_FLAG_FUSE_U8_LOAD,
    i.e. config 3 exactly as BASELINE states it (-p 2, uint8 load fused) and the same for fp32.
    Thresholds = about ten times the measured distributions (profiles/r02_q_pytest_gpu.txt, r03_*_pytest_gpu.txt), far inside
    north_star's 1e-4: fp32 pre-sharpen max 6e-7 .. 1e-6 measured -> 1e-5; sharpened "N" frames max 2e-6, p99.99 1.2e-6 ->
    2e-5 / 1.2e-5 and NO pixel above 1e-4; uniform noise max 8.5e-5 (the filter's sqrt has unbounded slope at 0: a handful
    of pixels whose 3x3 minimum is exactly 0 in fp64 amplify fp32 noise) -> 2e-4, p99.99 2.1e-6 -> 2.5e-5."""
    _check_full_size(W, H, precision, flags, dist)


def _check_full_size(W, H, precision, flags, dist, tagx=""):
    (pre, out, u8), (opre, oout, ou8) = _run(W, H, 2.0, precision, dist, flags=flags)
    tag = "%dx%d p%d flags%d %s%s" % (W, H, precision, flags, dist, tagx)
    if precision == 0:
        sp = _report(tag + " pre*u^2", (pre - opre) * 4, 1e-5)
        so = _report(tag + " out", out - oout, 1e-4)
        assert rel_l2(pre, opre) <= 2e-6
        assert sp["max"] <= 1e-5 and sp["p99.99"] <= 5e-6 and sp["count_above"] == 0
        assert rel_l2(out, oout) <= 1e-5
        if dist == "N":
            assert so["max"] <= 2e-5 and so["p99.99"] <= 1.2e-5 and so["count_above"] == 0
        else:
            assert so["max"] <= 2e-4 and so["p99.99"] <= 2.5e-5 and so["count_above"] <= 3
        d = np.abs(u8.astype(int) - ou8.astype(int))
        assert d.max() <= 1 and (d != 0).mean() <= 5e-4
    else:
        assert within_one_half_ulp(pre, opre).all()
        # in binary16 ulps of the output (ulp at 0.5..1 = 4.9e-4): the sharpen amplifies one-ulp input flips
        # (measured: p99 0, p99.99 one ulp = 9.8e-4, max 2e-3 .. 3.4e-3, 4e-6 .. 8e-5 of the pixels above one ulp)
        so = _report(tag + " out", out - oout, 2.0 ** -10)
        assert rel_l2(out, oout) <= 3e-4
        assert so["max"] <= 6e-3 and so["p99"] == 0 and so["p99.99"] <= 2e-3 and so["count_above"] <= 4e-4 * so["n"]


def _config1_rgb():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "no_upscaling_rgb.npz"))


@pytest.mark.parametrize("flags", [0, 2])
def test_config1_literal_image_api(flags):
    """BASELINE config 1: the decoded pixels of the reference's samples/no_upscaling.png (stb_image, 3 channels,
    VR:1362) -u 2 -p 0 -n 1 through the C ABI, float planes and u8 against the oracle."""
    d = _config1_rgb()
    (pre, out, u8), (opre, oout, ou8) = _run_rgb(d["rgb"], 2.0, 0, flags=flags)
    assert np.abs(oout[:, 1000:1064, 1800:1864] - d["out_crop"]).max() <= 1e-12       # the oracle build is sane
    so = _report("config1 no_upscaling.png flags%d out" % flags, out - oout, 1e-4)
    assert np.abs(pre - opre).max() * 4 <= 1e-5 and rel_l2(pre, opre) <= 2e-6
    assert so["p99.99"] <= 1.5e-5 and so["max"] <= 1e-4 and so["count_above"] == 0        # (measured 1.4e-6 / 9e-6)
    dd = np.abs(u8.astype(int) - ou8.astype(int))
    print("PARITY config1 u8: differing codes %.2e, max %d" % ((dd != 0).mean(), dd.max()))
    assert dd.max() <= 1 and (dd != 0).mean() <= 5e-4                                      # (measured 5e-5)


def test_full_size_properties():
    """Size-independent properties at the headline size: linearity in the input (pre-sharpen) and
    DC preservation (mean of every plane is kept by zero-padding the spectrum)."""
    from vkresample_amd import synth
    W, H = 2048, 1024
    a = synth.frame(1, W, H, "N").astype(np.float32) / 255
    b = synth.frame(2, W, H, "U").astype(np.float32) / 255
    pa = np.ascontiguousarray(a.transpose(2, 0, 1))
    pb = np.ascontiguousarray(b.transpose(2, 0, 1))
    with _up(W, H, 2.0, 0) as up:
        res = []
        for p in (pa, pb, (0.5 * pa + 0.25 * pb).astype(np.float32)):
            up.upload_planar(p)
            up.execute(1)
            res.append(up.download_presharpen().astype(np.float64) * 4)
    lin = 0.5 * res[0] + 0.25 * res[1]
    assert np.abs(res[2] - lin).max() <= 2e-5
    for r, p in zip(res[:2], (pa, pb)):
        assert np.abs(r.mean(axis=(1, 2)) - p.astype(np.float64).mean(axis=(1, 2))).max() <= 1e-6


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("pps", [1, 5, 6, 7, 256, 300, 1000])
def test_fused_sharpen_equals_unfused(precision, pps, monkeypatch):
    """The fused C2R+sharpen kernel (strips, one halo pair, explicit DC-leak, deferred last pixel, corner
    sample) against the two-launch path on the same frame, for strip lengths that do / do not divide the
    plane, cross plane boundaries, or swallow whole planes."""
    from vkresample_amd import FLAG_UNFUSED_SHARPEN
    from vkresample_amd import _lib
    monkeypatch.setenv("FFTUP_LIBRARY", _lib.KNOBS_LIB_PATH)       # (the knob exists in the test build of the library only)
    monkeypatch.setenv("FFTUP_EXPERIMENT", "pairs_per_strip=%d" % pps)
    (pre, out, u8), _ = _run(512, 256, 2.0, precision, "U", seed=3)
    (pre2, out2, u82), _ = _run(512, 256, 2.0, precision, "U", flags=FLAG_UNFUSED_SHARPEN, seed=3)
    if precision == 0:
        # different row pairing -> different fp32 rounding of the same numbers
        assert np.abs(out - out2).max() <= 1e-4
        assert rel_l2(out, out2) <= 2e-6
        # the quirk column x = uW-1 and the strip-boundary rows are where the bookkeeping lives
        assert np.abs(out[:, :, -1] - out2[:, :, -1]).max() <= 1e-4
    else:
        # the fused kernel's packed-binary16 sharpen (native reciprocal + one residual step, native square root) against
        # the exactly rounded per-operation sequence of k_sharpen_t: measured 1e-4 .. 8e-4 of the pixels differ, by one ulp
        assert np.abs(out - out2).max() <= 8e-3
        assert (out != out2).mean() <= 5e-3


@pytest.mark.parametrize("name", ["g16x8_u2_p0", "g20x12_u2_p0", "g20x12_u2_p1", "g64x32_u2_p0", "g64x32_u2_p2", "gsample64_u2_p0"])
def test_golden_vectors_gpu(name):
    """HIP path against the committed golden fixtures (tests/golden/make_golden.py)."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    precision = int(d["precision"])
    (pre, out, u8), _ = _run_rgb(d["rgb"], float(d["upscale"]), precision, float(d["sharpen"]))
    if precision == 1:
        assert np.abs(pre - d["pre"]).max() <= 1e-12 and np.abs(out - d["out"]).max() <= 1e-9
        assert np.abs(u8.astype(int) - d["u8"].astype(int)).max() <= 1
    elif precision == 0:
        measured("golden " + name, pre_max=np.abs(pre - d["pre"]).max() * 4, pre_l2=rel_l2(pre, d["pre"]),
                 out_max=np.abs(out - d["out"]).max(), out_l2=rel_l2(out, d["out"]))
        assert np.abs(pre - d["pre"]).max() * 4 <= 4e-6 and rel_l2(pre, d["pre"]) <= 2e-6                     # (measured 3.9e-7, 1.6e-7)
        assert np.abs(out - d["out"]).max() <= 1e-5 and rel_l2(out, d["out"]) <= 3e-6     # (7.9e-7, 3.0e-7)
        assert np.abs(u8.astype(int) - d["u8"].astype(int)).max() <= 1
    else:
        assert within_one_half_ulp(pre, d["pre"]).all()
        measured("golden " + name, out_max=np.abs(out - d["out"]).max(), out_diff_frac=(out != d["out"]).mean())
        assert np.abs(out - d["out"]).max() <= 4e-3 and (out != d["out"]).mean() <= 2e-3      # (7.3e-4, 1.7e-4)


@pytest.mark.parametrize("W,H", [(1920, 1080), (1280, 720)])
def test_mixed_radix_plans_equal_generic(W, H):
    """compile-time mixed-radix plans (1920x1080: 15*8*16 / 9*10*12 / 16*16*15; 1280x720: 5*16*16 / 9*8*10 / 16*16*10)
    vs the size-generic kernels on the same frame"""
    from vkresample_amd import FLAG_GENERIC_KERNELS
    with _up(W, H, 2.0, 0) as up:
        assert up.tuned
    (pre, out, u8), _ = _run(W, H, 2.0, 0, "N", seed=5)
    (pre2, out2, u82), _ = _run(W, H, 2.0, 0, "N", seed=5, flags=FLAG_GENERIC_KERNELS)
    assert np.abs(pre - pre2).max() * 4 <= 2e-6
    assert np.abs(out - out2).max() <= 1e-4


def test_timed_ring_and_profile_api():
    """measurement entry points: kernel durations are positive, ordered like the launches, and the timed batch
    produces the same pixels as the plain one"""
    from vkresample_amd import synth
    W, H = 512, 256
    with _up(W, H, 2.0, 0, ring=2) as up:
        for s in range(2):
            up.upload_rgb8(synth.frame(40 + s, W, H), slot=s)
        up.execute_ring(4, 0)
        ref = [up.download_planar(s) for s in range(2)]
        ms, km = up.execute_ring_timed(8, 0, 2)
        got = [up.download_planar(s) for s in range(2)]
        iso = up.profile_kernels(3)
        assert up.kernel_names[:3] == ["row_r2c", "col_fwd_pad_inv", "row_c2r_sharpen"]
    # (isolated durations are net of an empty event pair's own cost: a 4-us kernel of this small size may come out as 0)
    assert ms > 0 and all(k > 0 for k in km[:3]) and all(k >= 0 for k in iso[:3])
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)


def test_u8_wrap_flag():
    """FFTUP_FLAG_U8_WRAP reproduces the x86 behaviour of the reference's C cast (VR:1715) where the sharpened value
    leaves [0,1]; the default saturates.  Both agree with the oracle's two store modes."""
    from vkresample_amd import FLAG_U8_WRAP, synth
    rgb = synth.frame(8, 128, 64, "U")                      # uniform noise: plenty of overshoot after sharpening
    outs = {}
    for flags in (0, FLAG_U8_WRAP):
        with _up(128, 64, 2.0, 0, 0.2, 0, flags) as up:
            up.upload_rgb8(rgb)
            up.execute(1)
            outs[flags] = (up.download_rgb8(), up.download_planar().astype(np.float64))
    sat, planes = outs[0]
    wrap, _ = outs[FLAG_U8_WRAP]
    x = planes.transpose(1, 2, 0) * 255.0
    inside = (x >= 0) & (x < 255)
    assert np.array_equal(sat[inside], wrap[inside])
    lo, hi = x < 0, x >= 256
    assert lo.any() or hi.any()
    assert (sat[lo] == 0).all() and (sat[x >= 255] == 255).all()
    assert np.array_equal(wrap[lo], (np.trunc(x[lo]).astype(np.int64) & 0xFF).astype(np.uint8))
    if hi.any():
        assert np.array_equal(wrap[hi], (np.trunc(x[hi]).astype(np.int64) & 0xFF).astype(np.uint8))


def test_largest_r2c_size_vs_oracle():
    """uW = 8192 is the largest width the reference's R2C path accepts (VkResample.cpp:1424)."""
    (pre, out, u8), (opre, oout, ou8) = _run(4096, 64, 2.0, 0, "N", seed=9)
    measured("largest_r2c", pre_l2=rel_l2(pre, opre), pre_max=np.abs(pre - opre).max() * 4, out_l2=rel_l2(out, oout),
             out_max=np.abs(out - oout).max())
    assert rel_l2(pre, opre) <= 2e-6 and np.abs(pre - opre).max() * 4 <= 6e-6                  # (measured 1.6e-7, 5.4e-7)
    assert rel_l2(out, oout) <= 4e-6 and np.abs(out - oout).max() <= 2e-5     # (4.0e-7, 1.7e-6)


@pytest.mark.parametrize("W,H,u,precision,flags", [(4608, 64, 2.0, 0, 0), (4608, 64, 2.0, 0, 2), (3072, 32, 3.0, 0, 0),
                                                   (2304, 32, 2.0, 1, 0), (6144, 16, 1.5, 0, 0),
                                                   (4608, 16, 2.0, 2, 0), (4608, 16, 2.0, 2, 2), (3072, 8, 3.0, 2, 2),      # (-p 2: the oracle's binary16 sharpen is slow)
                                                   # rows beyond ~9600 points: one LDS buffer, in place (VERDICT r2 missing 2)
                                                   (5120, 16, 2.0, 0, 0), (6144, 16, 2.0, 0, 2), (8192, 8, 2.0, 0, 0), (7168, 8, 2.0, 2, 2),
                                                   (7680, 8, 2.0, 0, 0), (10240, 8, 1.5, 0, 0)])
def test_non_r2c_complex_path_vs_oracle(W, H, u, precision, flags):
    """beyond the R2C limit (uW > 8192; > 4096 for -p 1) the reference runs full complex transforms with a
    four-quadrant shift (VR:527-546) and sharpens the modulus of the complex image; the imaginary input parts, which the
    reference leaves uninitialised, are defined as 0.  The pre-sharpen tap returns the real part."""
    assert O.uses_complex_path(W, H, u, precision)
    (pre, out, u8), (opre, oout, ou8) = _run(W, H, u, precision, "N", flags=flags, seed=21)
    usq = u * u
    if precision == 0:
        measured("non_r2c %dx%d u%g" % (W, H, u), pre_l2=rel_l2(pre, opre), pre_max=np.abs(pre - opre).max() * usq, out_l2=rel_l2(out, oout))
        assert rel_l2(pre, opre) <= 2e-6 and np.abs(pre - opre).max() * usq <= 6e-6               # (measured <= 1.8e-7, 5.2e-7)
        so = _report("non-R2C %dx%d u%g out" % (W, H, u), out - oout, 1e-4)
        assert rel_l2(out, oout) <= 5e-6 and so["max"] <= 1.5e-5 and so["p99.99"] <= 1e-5     # (4.3e-7, 1.4e-6, 1.1e-6)
    elif precision == 2:
        # -p 2 beyond the R2C limit (VERDICT r2 missing 1): half input and half complex pre-sharpen image around fp32
        # transforms (VR:1420-1424, VF:7282-7292), the complex sharpen in binary16 arithmetic (VR:865-907 with f16vec2)
        assert within_one_half_ulp(pre, opre).all()
        so = _report("non-R2C -p 2 %dx%d u%g out" % (W, H, u), out - oout, 2.0 ** -10)
        assert so["max"] <= 8e-3 and so["p99"] == 0 and so["p99.99"] <= 3e-3
        d = np.abs(u8.astype(int) - ou8.astype(int))
        assert d.max() <= 2 and (d > 1).mean() <= 1e-3
        return
    else:
        assert np.abs(pre - opre).max() <= 1e-12 and np.abs(out - oout).max() <= 1e-9
    d = np.abs(u8.astype(int) - ou8.astype(int))
    assert d.max() <= 1 and (d != 0).mean() <= 5e-3


def test_non_r2c_limits():
    import vkresample_amd as v
    with pytest.raises(v.FftupError) as e:           # 2 * 32771 (a prime): not 2,3,5,7-smooth
        v.Upscaler(32771 * 2, 16, 1.0)
    assert e.value.code in (1, 2)
    with _up(5120, 16, 2.0) as up:                   # 10240-point rows: the one-buffer form
        assert up.kernel_names == ["row_c2c", "col_fwd_pad_inv", "row_c2c_inv", "sharpen"] and not up.tuned
    with _up(4608, 16, 2.0, 2) as up:                # -p 2 beyond the R2C limit
        assert up.kernel_names[0] == "row_c2c"
    with _up(4608, 16, 2.0) as up:
        assert up.kernel_names == ["row_c2c", "col_fwd_pad_inv", "row_c2c_inv", "sharpen"] and not up.tuned
    for W, u, p, what in ((9216, 2.0, 0, "inverse rows in four steps 128*144"), (8064, 2.0, 0, "inverse rows in four steps 112*144"),
                          (2560, 2.0, 1, "inverse rows in four steps 64*80"), (17280, 1.0, 0, "forward rows in four steps 120*144"),
                          (8748, 2.0, 0, "inverse rows in four steps 54*324 (tiles of 4 / 2)")):
        with _up(W, 16, u, p) as up:               # beyond one LDS buffer: four steps (refused until round 4)
            assert up.kernel_names[0] == "row_c2c" and not up.tuned and what in up.description, up.description
    with _up(16, 4900, 3.0) as up:
        assert "forward columns in four steps 70*70" in up.description and "inverse columns in four steps" in up.description, up.description
    with _up(16, 4900, 2.0) as up:                 # u = 2: the polyphase column kernel needs ONE buffer of 4900 points (round 5; four steps before)
        assert "polyphase column pass" in up.description and "four steps" not in up.description, up.description


FOUR_STEP = [(9216, 8, 2.0, 0, 0),       # inverse rows of 18432 = 128 * 144 points in four steps, forward rows (9216) in one launch
             (9216, 8, 2.0, 0, 2), (9216, 8, 2.0, 2, 2),    # ... from the uint8 image; -p 2
             (17280, 4, 1.0, 0, 0),      # -u 1: forward AND inverse rows of 17280 = 2^7 3^3 5 points in four steps
             (8064, 8, 2.0, 0, 0),       # 16128 = 2^8 * 63: the one-buffer form has no radix-7 stage that long
             (20000, 4, 1.5, 0, 0),      # 30000-point inverse rows, 20000-point forward rows
             (2560, 8, 2.0, 1, 0),       # -p 1: two buffers of 5120 double2 do not fit
             (8748, 4, 2.0, 0, 0)]       # 17496 = 2^3 3^7 = 54 * 324: no factor pair with 4 | both -- pass A in tiles of 4, pass B in tiles of 2


@pytest.mark.parametrize("W,H,u,precision,flags", FOUR_STEP)
def test_four_step_rows_vs_oracle(W, H, u, precision, flags):
    """Non-R2C rows beyond one LDS buffer (16 384 points; ~4 800 for -p 1): the reference switches to multi-upload plans with a
    transposition through a temporary buffer (VF:4773-4992, 2290-2388, 6562-6576); here k_row4_a / k_row4_b run the row as
    N1 x N2 in two launches through HBM.  Same bars as the one-launch non-R2C rows."""
    assert O.uses_complex_path(W, H, u, precision)
    (pre, out, u8), (opre, oout, ou8) = _run(W, H, u, precision, "N", flags=flags, seed=23)
    usq = u * u
    if precision == 0:
        measured("four_step %dx%d u%g" % (W, H, u), pre_l2=rel_l2(pre, opre), pre_max=np.abs(pre - opre).max() * usq, out_l2=rel_l2(out, oout),
                 out_max=np.abs(out - oout).max())
        assert rel_l2(pre, opre) <= 2e-6 and np.abs(pre - opre).max() * usq <= 6e-6
        assert rel_l2(out, oout) <= 5e-6 and np.abs(out - oout).max() <= 2e-5      # (measured <= 1.9e-7, 4.8e-7; 4.3e-7, 1.4e-6)
    elif precision == 2:
        assert within_one_half_ulp(pre, opre).all()
        so = _report("four-step -p 2 %dx%d u%g out" % (W, H, u), out - oout, 2.0 ** -10)
        assert so["max"] <= 8e-3 and so["p99"] == 0 and so["p99.99"] <= 3e-3
    else:
        assert np.abs(pre - opre).max() <= 1e-12 and np.abs(out - oout).max() <= 1e-9
    d = np.abs(u8.astype(int) - ou8.astype(int))
    assert d.max() <= (2 if precision == 2 else 1)


TALL = [(16, 4900, 2.0, 0, 0),          # uH = 9800: two Stockham buffers of one column do not fit 160 KB; 4900 = 70 * 70, 9800 = 98 * 100
        (16, 4900, 2.0, 0, 2), (32, 4900, 2.0, 2, 2),      # (u = 2: since round 5 the polyphase column kernel, ONE buffer of 4900 points, no four steps)
        (16, 4900, 3.0, 0, 0),          # uH = 14700: both column transforms in four steps
        (16, 2500, 3.0, 1, 0),          # -p 1: uH = 7500 in double2, four steps
        (20, 9800, 1.5, 0, 0),          # H itself beyond one column's LDS, uH = 14700 = 105 * 140, non-integer factor
        (16, 2500, 2.0, 1, 0),          # -p 1: uH = 5000 in double2
        (2100, 2500, 2.0, 1, 0)]        # ... on the non-R2C path (uW = 4200 > 4096 for -p 1)


@pytest.mark.parametrize("W,H,u,precision,flags", TALL)
def test_four_step_columns_vs_oracle(W, H, u, precision, flags):
    """Columns longer than the LDS (uH beyond ~9 600, ~4 800 for -p 1; refused until round 4; the reference: multi-upload plans,
    VF:4773-4992): the spectrum keeps tiles of ONE column and both column transforms run through k_row4_a / k_row4_b -- forward in
    place, inverse with the y half of the shift and the read guard in the load.  Same bars as every other size-generic plan."""
    (pre, out, u8), (opre, oout, ou8) = _run(W, H, u, precision, "N", flags=flags, seed=29)
    usq = u * u
    if precision == 0:
        measured("tall %dx%d u%g" % (W, H, u), pre_l2=rel_l2(pre, opre), pre_max=np.abs(pre - opre).max() * usq, out_l2=rel_l2(out, oout),
                 out_max=np.abs(out - oout).max())
        assert rel_l2(pre, opre) <= 2e-6 and np.abs(pre - opre).max() * usq <= 6e-6
        assert rel_l2(out, oout) <= 5e-6 and np.abs(out - oout).max() <= 2e-5
    elif precision == 2:
        assert within_one_half_ulp(pre, opre).all()
        so = _report("tall -p 2 %dx%d u%g out" % (W, H, u), out - oout, 2.0 ** -10)
        assert so["max"] <= 8e-3 and so["p99"] == 0 and so["p99.99"] <= 3e-3
    else:
        assert np.abs(pre - opre).max() <= 1e-12 and np.abs(out - oout).max() <= 1e-9
    d = np.abs(u8.astype(int) - ou8.astype(int))
    assert d.max() <= (2 if precision == 2 else 1)


def test_4k_to_8k_properties():
    """4096x2048 -> 8192x4096 (size-generic kernels, 0.4 GB of output): DC preservation and determinism."""
    from vkresample_amd import synth
    W, H = 4096, 2048
    rgb = synth.frame(12, W, H, "N")
    with _up(W, H, 2.0, 0) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        pre = up.download_presharpen().astype(np.float64) * 4
        out1 = up.download_planar()
        up.execute(2)
        out2 = up.download_planar()
    want = (rgb.astype(np.float32) / np.float32(255)).astype(np.float64).mean(axis=(0, 1))
    assert np.abs(pre.mean(axis=(1, 2)) - want).max() <= 1e-6
    assert np.array_equal(out1, out2)
    assert out1.min() > -0.05 and out1.max() < 1.05


@pytest.mark.parametrize("W,H,precision,flags,ring,pinned", [(128, 64, 0, 0, 3, True), (512, 256, 0, 0, 2, False),
                                                             (512, 256, 2, 2, 4, True), (60, 36, 0, 0, 1, True)])
def test_host_streamed_queue_equals_blocking_calls(W, H, precision, flags, ring, pinned):
    """fftup_submit_rgb8 / fftup_wait: every frame of a queue deeper than the ring comes back
    byte-identical to upload_rgb8 -> execute -> download_rgb8 of the same frame."""
    import vkresample_amd as v
    from vkresample_amd import synth
    n = 3 * ring + 1
    frames = [synth.frame(100 + k, W, H, "N" if k % 2 else "U") for k in range(n)]
    with _up(W, H, 2.0, precision, flags=flags, ring=ring) as up:
        want = []
        for f in frames:
            up.upload_rgb8(f)
            up.execute(1)
            want.append(up.download_rgb8())
        if pinned:
            pin_in, pin_out = v.PinnedArray((n, H, W, 3)), v.PinnedArray((n, 2 * H, 2 * W, 3))
            ins, outs = pin_in.array, pin_out.array
        else:
            ins, outs = np.empty((n, H, W, 3), np.uint8), np.empty((n, 2 * H, 2 * W, 3), np.uint8)
        outs[:] = 7
        for k, f in enumerate(frames):
            ins[k] = f
        tickets = [up.submit_rgb8(ins[k], outs[k]) for k in range(n)]
        assert tickets == list(range(n))
        up.wait(tickets[0])                        # long since retired (slot reused)
        up.wait(tickets[-1])
        up.drain()
        for k in range(n):
            assert np.array_equal(outs[k], want[k]), k
        # the queue keeps working after a drain, tickets keep counting
        t = up.submit_rgb8(ins[1], outs[0])
        assert t == n
        up.wait(t)
        assert np.array_equal(outs[0], want[1])
        with pytest.raises(v.FftupError) as e:
            up.wait(t + 1)
        assert e.value.code == 1
        if pinned:
            pin_in.close()
            pin_out.close()


@pytest.mark.parametrize("W,H,precision,flags,ring", [(256, 128, 0, 0, 4), (512, 256, 2, 6, 16), (240, 126, 0, 0, 2)])
def test_one_plan_fed_by_several_host_threads(W, H, precision, flags, ring):
    """fftup_submit_rgb8 / fftup_wait of ONE plan from several host threads at once (the batched CLI: codec workers sharing the
    GPU's plan): six threads, each double-buffered over its own page-locked buffers like the CLI's loop, 7 frames each -- every
    frame comes back byte-identical to the blocking calls, tickets are issued exactly once."""
    import threading
    import vkresample_amd as v
    from vkresample_amd import synth
    T, per = 6, 7
    frames = [synth.frame(300 + k, W, H, "N" if k % 3 else "U") for k in range(T * per)]
    with _up(W, H, 2.0, precision, flags=flags, ring=ring) as up:
        want = []
        for f in frames:
            up.upload_rgb8(f)
            up.execute(1)
            want.append(up.download_rgb8())
        got = [None] * len(frames)
        tickets = [[] for _ in range(T)]
        errors = []

        def worker(t):
            try:
                pin, pout = v.PinnedArray((2, H, W, 3)), v.PinnedArray((2, 2 * H, 2 * W, 3))
                tk = [None, None]
                mine = list(range(t, T * per, T))                  # the stripe f*T + t
                for i, g in enumerate(mine):
                    pin.array[i & 1] = frames[g]
                    tk[i & 1] = up.submit_rgb8(pin.array[i & 1], pout.array[i & 1])
                    tickets[t].append(tk[i & 1])
                    if i > 0:
                        up.wait(tk[(i - 1) & 1])
                        got[mine[i - 1]] = pout.array[(i - 1) & 1].copy()
                up.wait(tk[(len(mine) - 1) & 1])
                got[mine[-1]] = pout.array[(len(mine) - 1) & 1].copy()
                pin.close()
                pout.close()
            except Exception as e:                                 # noqa: BLE001 (reported by the main thread)
                errors.append((t, repr(e)))

        th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errors, errors
        assert sorted(sum(tickets, [])) == list(range(T * per))
        for k in range(len(frames)):
            assert np.array_equal(got[k], want[k]), k
        up.drain()


@pytest.mark.parametrize("W,H,u", [(16, 8, 2.0), (60, 42, 2.0), (24, 16, 3.0), (16, 8, 1.5), (32, 16, 1.25), (256, 128, 2.0),
                                   (240, 270, 2.0), (1024, 512, 2.0), (2048, 64, 2.0), (64, 2048, 2.0), (96, 1200, 2.5)])
@pytest.mark.parametrize("dist", ["U", "N"])
def test_fp64_parity(W, H, u, dist):
    """-p 1: double buffers and double arithmetic end to end; the oracle is fp64 too, so the two
    agree to rounding: 1e-12 before the sharpen, 1e-9 after it (sqrt(min) amplifies near 0, see the fp32 test)."""
    (pre, out, u8), (opre, oout, ou8) = _run(W, H, u, 1, dist)
    assert pre.dtype == np.float64
    assert np.abs(pre - opre).max() <= 1e-12
    assert np.abs(out - oout).max() <= 1e-9
    d = u8.astype(int) - ou8.astype(int)
    assert np.abs(d).max() <= 1 and (d != 0).mean() <= 1e-4      # trunc(255*x) flips where 255*x is an integer +- 1 ulp


def test_fp64_sharpen_against_the_ieee_sequence_in_ulps(monkeypatch):
    """the -p 1 sharpen forms its quotients and its root from v_rcp_f64 / v_rsq_f64 seeds and Newton steps
    (sharpen_eval_f64) instead of IEEE division sequences.  Against the same kernel with the shader's own divisions and root
    (k_sharpen_f64<.., EXACT>, test build of the library) on the same pre-sharpen image: an explicit bound in units of the last
    place, on frames whose 3x3 minima reach 0 and maxima reach 1 (black and white blocks: n -> 0, the root's steep end; d -> 1)."""
    from vkresample_amd import _lib, synth
    W, H = 256, 128
    rgb = synth.frame(11, W, H, "N").copy()
    rgb[8:40, 16:80] = 0                                     # mn = 0 over whole neighbourhoods
    rgb[60:100, 100:200] = 255                               # mx = 1 (clamped)
    rgb[20:30, 150:160] = np.random.default_rng(1).integers(0, 3, (10, 10, 3))       # tiny non-zero minima
    monkeypatch.setenv("FFTUP_LIBRARY", _lib.KNOBS_LIB_PATH)
    res = []
    for exact in ("0", "1"):
        monkeypatch.setenv("FFTUP_EXPERIMENT", "f64_exact_sharpen=" + exact)
        with _up(W, H, 2.0, 1) as up:
            up.upload_rgb8(rgb)
            up.execute(1)
            res.append((up.download_presharpen().copy(), up.download_planar().copy()))
    assert np.array_equal(res[0][0], res[1][0])              # the same image goes into both filters
    fast, exact = res[0][1], res[1][1]
    assert np.isfinite(fast).all() and np.isfinite(exact).all()
    assert 4.0 * np.abs(res[0][0]).min() < 1e-4 and 4.0 * res[0][0].max() > 1.0       # taps |u^2 g| near 0 and clamped at 1 both occur
    # The output is (C + scale * s4) / (1 + 4 scale) with scale < 0: where the two terms of the numerator nearly cancel, the result is
    # small and an error of one unit in the last place of the TERMS is thousands of units of the result's own.  So: in units of
    # the last place of the filter's operands (values in [0, 1]: 2^-53), and in the result's own units where it is not small
    err = np.abs(fast - exact)
    u1 = err / 2.0 ** -53
    own = err[np.abs(exact) >= 0.25] / np.spacing(np.abs(exact[np.abs(exact) >= 0.25]))
    print("MEASURED fp64 sharpen vs IEEE sequence: max %.1f units of 2^-53, %.3f %% of the pixels differ; results >= 0.25: max %.1f ulp of their own"
          % (u1.max(), 100.0 * (err > 0).mean(), own.max()))
    assert u1.max() <= 16.0 and own.max() <= 8.0, (u1.max(), own.max())
    # and the IEEE form against the oracle: the same sequence of operations, to the last few bits
    opre, oout, _ = O.upscale_rgb8(rgb, 2.0, 1, 0.2)
    assert np.abs(exact - oout).max() <= 1e-9


def test_fp64_planar_input_and_limits():
    import vkresample_amd as v
    rng = np.random.default_rng(5)
    planes = rng.random((3, 36, 60))
    with _up(60, 36, 2.0, 1) as up:
        up.upload_planar(planes)
        assert np.array_equal(up.download_input_planar(), planes)
        up.execute(2)
        pre, out = up.download_presharpen(), up.download_planar()
    opre, oout = O.upscale_planes(planes, 2.0, 1)[:2]
    assert np.abs(pre - opre).max() <= 1e-12 and np.abs(out - oout).max() <= 1e-9
    with v.Upscaler(4096, 16, 2.0, 1) as up:           # complexSizeCalc = 16 halves the R2C limit (VR:1424): the non-R2C path, its
        assert up.kernel_names[0] == "row_c2c"         # 8192-point double2 rows in four steps (refused until round 4)
    # double vs single on the same frame: they differ by fp32 rounding only
    (pre64, _, _), _ = _run(256, 128, 2.0, 1, "N", seed=3)
    (pre32, _, _), _ = _run(256, 128, 2.0, 0, "N", seed=3)
    assert 1e-9 < np.abs(pre64 - pre32).max() < 1e-5


def test_fp64_host_streamed_queue():
    from vkresample_amd import synth
    W, H = 128, 64
    frames = [synth.frame(300 + k, W, H) for k in range(5)]
    with _up(W, H, 2.0, 1, ring=2) as up:
        outs = np.zeros((5, 2 * H, 2 * W, 3), np.uint8)
        ins = np.stack(frames)
        for k in range(5):
            up.submit_rgb8(ins[k], outs[k])
        up.drain()
    for k in range(5):
        _, _, ou8 = O.upscale_rgb8(frames[k], 2.0, 1)
        d = outs[k].astype(int) - ou8.astype(int)
        assert np.abs(d).max() <= 1 and (d != 0).mean() <= 1e-4


@pytest.mark.parametrize("flags", [0, 4])
@pytest.mark.parametrize("name", ["car", "close_people", "distant_people", "skyscraper", "trees"])
def test_hip_path_reproduces_reference_output_crops(name, flags):
    """The product against the reference's OWN pixels (tests/golden/make_readme_crops.py): crops of the images
    VkResample produced for its README, with the exact input of the crop window.  flags 0: size-specialised + fused
    kernels (512x512), 4: size-generic kernels."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readme_%s.npz" % name))
    with _up(512, 512, 2.0, 0, 0.2, 0, flags) as up:
        up.upload_rgb8(d["rgb"])
        up.execute(1)
        u8 = up.download_rgb8()
    # every panel pixel outside the label corner and a 12-pixel border (O.readme_panel_mask), same bounds as the oracle's test
    st = O.readme_panel_stats(u8, d)
    print("README %s flags%d HIP: %s" % (name, flags, st))
    assert st["mean"] <= 0.35 and st["p99"] <= 2 and st["p99.9"] <= 3 and st["max"] <= 5, st


U8_STORE_CASES = [(2048, 1024, 0, 0), (2048, 1024, 2, 2), (1920, 1080, 0, 2), (1280, 720, 2, 2), (512, 256, 0, 1), (1000, 1000, 0, 0),
                  (640, 480, 2, 2), (1024, 512, 0, 0)]


@pytest.mark.parametrize("W,H,precision,flags", U8_STORE_CASES)
def test_fused_u8_store_equals_planes_plus_conversion(W, H, precision, flags):
    """FFTUP_FLAG_FUSE_U8_STORE (SURVEY 8 f3 as written): the fused C2R+sharpen kernel stores the interleaved 8-bit image
    itself.  Same bytes, all of them, as the float / half planes followed by the conversion launch (k_pack_u8) -- for the
    ahead-of-time plans (2048x1024, 1920x1080, 1280x720, 512x256), plans specialised at plan time (1000x1000, 640x480), the
    wrapping store (flag 1) -- and within one code of the oracle (BASELINE configs 2, 3, 4); no float planes exist."""
    import vkresample_amd as v
    from vkresample_amd import FLAG_FUSE_U8_STORE, synth
    rgb = synth.frame(31, W, H, "U" if flags & 1 else "N")
    with _up(W, H, 2.0, precision, 0.2, 0, flags) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        ref = up.download_rgb8()
        assert not up.u8_store
    with _up(W, H, 2.0, precision, 0.2, 0, flags | FLAG_FUSE_U8_STORE) as up:
        assert up.u8_store and "8-bit RGB store" in up.description
        up.upload_rgb8(rgb)
        up.execute(2)
        got = up.download_rgb8()
        with pytest.raises(v.FftupError):
            up.download_planar()
        assert up.output_checksum(0) == int(np.frombuffer(got.tobytes(), dtype=np.uint32).astype(np.uint64).sum())
    # Same conversion of the same sharpened values -- but the store variant cuts the planes into strips of their own (one plane
    # per strip, the three planes' strips of the same rows on one XCD), and where a cut falls decides which rows share a complex
    # transform and its rounding (test_fused_output_independent_of_strip_length: <= 5e-6 / a binary16 ulp): a value that close to
    # k/255 may land on the other side.  Measured: 2 bytes of 25 M (fp32), none where the strips coincide.
    d = np.abs(got.astype(int) - ref.astype(int))
    print("U8STORE %dx%d p%d flags %d: %d of %d bytes differ, max %d" % (W, H, precision, flags, int((d != 0).sum()), d.size, int(d.max())))
    if flags & 1:       # (wrapping store: a value a rounding below 0 wraps to 255)
        assert (d != 0).mean() <= (1e-6 if precision == 0 else 1e-4)
    else:
        assert d.max() <= 1 and (d != 0).mean() <= (1e-6 if precision == 0 else 1e-4), (np.argwhere(got != ref)[:5], (got != ref).sum())
    if W * H <= 2048 * 1024 and not (flags & 1):
        _, _, ou8 = O.upscale_rgb8(rgb, 2.0, precision, 0.2)
        d = np.abs(got.astype(int) - ou8.astype(int))
        assert d.max() <= (1 if precision == 0 else 2)


def test_fused_u8_store_host_streamed_and_unfused_fallback():
    """the host-streamed queue with the fused 8-bit store (no conversion launch between the kernels and the D2H copy), and a
    plan without a fused kernel: the flag is ignored, fftup_info says so, the bytes are the same"""
    import vkresample_amd as v
    from vkresample_amd import FLAG_FUSE_U8_LOAD, FLAG_FUSE_U8_STORE, FLAG_GENERIC_KERNELS, synth
    W, H, n = 1024, 512, 6
    frames = [synth.frame(80 + k, W, H) for k in range(n)]
    outs = []
    for fl in (FLAG_FUSE_U8_LOAD, FLAG_FUSE_U8_LOAD | FLAG_FUSE_U8_STORE, FLAG_GENERIC_KERNELS | FLAG_FUSE_U8_STORE):
        with v.Upscaler(W, H, 2.0, 0, 0.2, 0, fl, ring=3) as up, v.PinnedArray((n, H, W, 3)) as pi, v.PinnedArray((n, 2 * H, 2 * W, 3)) as po:
            assert up.u8_store == (fl == (FLAG_FUSE_U8_LOAD | FLAG_FUSE_U8_STORE))
            for k in range(n):
                pi.array[k] = frames[k]
                up.submit_rgb8(pi.array[k], po.array[k])
            up.drain()
            outs.append(po.array.copy())
    d01 = np.abs(outs[0].astype(int) - outs[1].astype(int))     # (strips of its own: see test_fused_u8_store_equals_planes_plus_conversion)
    assert d01.max() <= 1 and (d01 != 0).mean() <= 1e-6
    d = np.abs(outs[2].astype(int) - outs[0].astype(int))
    assert d.max() <= 1 and (d != 0).mean() <= 1e-3          # size-generic kernels: other fp32 roundings, same pixels


def test_plans_in_concurrent_host_threads():
    """one plan per host thread, no shared mutable state (the reference's -numthreads model, VR:1282-1320, 1959-1969):
    four threads with different configurations run interleaved on one device and reproduce their single-threaded
    results bit for bit; errors stay thread-local."""
    import threading
    import vkresample_amd as v
    from vkresample_amd import synth
    cfgs = [(512, 256, 0, 0), (240, 126, 0, 0), (512, 256, 2, 2), (128, 64, 1, 0)]
    frames = [[synth.frame(700 + 10 * t + k, W, H) for k in range(6)] for t, (W, H, _, _) in enumerate(cfgs)]

    def run(t, out):
        W, H, p, flags = cfgs[t]
        res = []
        with v.Upscaler(W, H, 2.0, p, 0.2, 0, flags, ring=2) as up:
            for rep in range(3):
                for k, f in enumerate(frames[t]):
                    up.upload_rgb8(f, slot=k % 2)
                    up.execute_ring(1, k % 2)
                    if rep == 2:
                        res.append(up.download_rgb8(k % 2))
            try:
                v.Upscaler(2 * 11 * 64, 64)                 # a failing call in this thread ...
            except v.FftupError as e:
                res.append(e.code)
        out[t] = res

    want = [None] * 4
    for t in range(4):
        run(t, want)
    got = [None] * 4
    th = [threading.Thread(target=run, args=(t, got)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for t in range(4):
        assert got[t][-1] == 2 and want[t][-1] == 2
        for a, b in zip(got[t][:-1], want[t][:-1]):
            assert np.array_equal(a, b)


def _knobs_lib():
    from vkresample_amd import _lib
    return _lib.KNOBS_LIB_PATH


def _run_env(env, W, H, precision, dist="N", flags=0):
    """Output planes of one frame with plan-creation environment switches set (read by fftup_plan_create)."""
    from vkresample_amd import synth
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        rgb = synth.frame(3, W, H, dist)
        with _up(W, H, 2.0, precision, 0.2, 0, flags) as up:
            up.upload_rgb8(rgb)
            up.execute(1)
            return up.download_planar().copy()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("W,H", [(512, 256), (2048, 1024), (1920, 1080), (1280, 720)])
@pytest.mark.parametrize("precision", [0, 2])
def test_fused_output_independent_of_strip_length(W, H, precision):
    """The fused C2R+sharpen kernel cuts the frame into strips of row pairs; every strip recomputes one halo pair, keeps
    the previous pair's rows in registers, defers its last pixel per row pair and takes the corner sample of its last row
    from a reduction.  None of that may depend on where the cuts fall: strips of 3, 5, 7 and 50 pairs (the last one
    crossing plane boundaries) agree with the default (one strip per compute unit) to rounding.  Not bit for bit: the
    first strip of a plane pairs rows (0,1), (2,3) ..., the others (odd, even), two rows of a pair share one complex
    transform and its rounding errors, and the corner sample comes from a sum instead of the transform -- measured
    <= 1.8e-6 (fp32), 61 pixels in 1.5 M one or two binary16 ulps apart (-p 2).  A wrong halo, tap or cut costs >= 1e-3."""
    ref = _run_env({}, W, H, precision).astype(np.float64)
    for pairs in ((1, 2, 3, 5, 7, 50) if W == 512 else (3, 5, 7, 50)):
        got = _run_env({"FFTUP_EXPERIMENT": "pairs_per_strip=%d" % pairs, "FFTUP_LIBRARY": _knobs_lib()}, W, H, precision).astype(np.float64)
        d = np.abs(ref - got)
        if precision == 0:
            assert d.max() <= 5e-6, "pairs_per_strip = %d: %g" % (pairs, d.max())
        else:
            assert d.max() <= 4e-3 and (d != 0).mean() <= 2e-4, "pairs_per_strip = %d: %g, %g" % (pairs, d.max(), (d != 0).mean())


@pytest.mark.parametrize("W,H,precision,flags", [(256, 128, 0, 0), (640, 480, 0, 2), (2048, 1024, 2, 2), (2048, 1024, 0, 32), (1920, 1080, 0, 0),
                                                 (16, 8, 1, 0), (9216, 8, 0, 0), (512, 256, 0, 8)])
def test_overlapped_iterations_are_bit_identical_to_the_ordered_form(W, H, precision, flags, monkeypatch):
    """fftup_execute(n) runs its n identical iterations in order on one stream -- the reference's one command buffer with a barrier
    behind every stage (VR:1260-1265, VR:1217, vkFFT.h:7678).  FFTUP_FLAG_OVERLAP_ITERATIONS (extension) lets them alternate on the
    plan's streams (own spectra, own scratch output per stream): the same kernels with the same arguments on the same input, so
    output slot 0 holds the bits ONE iteration leaves (n = 1 runs alone on stream 0), for n = 2, 3, 35, on plans with and without
    a ring, fused, unfused (FFTUP_FLAG_UNFUSED_SHARPEN), 8-bit store (32), -p 1, four-step rows.  The ordered form gives the same
    frame: bit for bit wherever the result does not depend on the fused kernel's strip length (a plan without a ring and without
    the flag cuts two strips per compute unit), to rounding where it does."""
    from vkresample_amd import FLAG_FUSE_U8_STORE, FLAG_OVERLAP_ITERATIONS, FLAG_SEQUENTIAL_EXECUTE, synth
    rgb = synth.frame(70, W, H)
    get = (lambda up: up.download_rgb8(0).copy()) if flags & FLAG_FUSE_U8_STORE else (lambda up: up.download_planar(0).copy())
    res = {}
    for ring in (1, 3):
        with _up(W, H, 2.0, precision, 0.2, 0, flags | FLAG_OVERLAP_ITERATIONS, ring=ring) as up:
            up.upload_rgb8(rgb)
            outs = []
            for n in (1, 2, 3, 35, 1):
                ms = up.execute(n)
                assert ms > 0
                outs.append(get(up))
            pre = up.download_presharpen().copy() if not flags & FLAG_FUSE_U8_STORE else None
            for o in outs[1:]:
                assert np.array_equal(outs[0], o)
            res[ring] = (outs[0], pre)
    assert np.array_equal(res[1][0], res[3][0])
    # a ring and no flag: ordered iterations on a plan laid out for overlapping frames -- the same cuts, the same bits
    with _up(W, H, 2.0, precision, 0.2, 0, flags, ring=3) as up:
        up.upload_rgb8(rgb)
        up.execute(3)
        assert np.array_equal(get(up), res[3][0])
    with _up(W, H, 2.0, precision, 0.2, 0, flags) as up:                 # the default: ordered iterations, no ring
        up.upload_rgb8(rgb)
        up.execute(5)
        seq, seq_pre = get(up), (up.download_presharpen().copy() if not flags & FLAG_FUSE_U8_STORE else None)
        fused = up.kernel_names[3] == "-"                               # C2R and sharpen in one launch: strips
    if seq_pre is not None:
        assert np.array_equal(seq_pre, res[1][1])                        # the transforms do not know about strips
    if fused:
        d = np.abs(seq.astype(np.float64) - res[1][0].astype(np.float64))
        assert d.max() <= (1 if flags & FLAG_FUSE_U8_STORE else 5e-6 if precision == 0 else 4e-3)
    else:
        assert np.array_equal(seq, res[1][0])
    with _up(W, H, 2.0, precision, 0.2, 0, flags | FLAG_SEQUENTIAL_EXECUTE) as up:     # (the flag of 0.6 and earlier: accepted, no effect)
        up.upload_rgb8(rgb)
        up.execute(2)
        assert np.array_equal(get(up), seq)
    monkeypatch.setenv("FFTUP_STREAMS", "1")
    with _up(W, H, 2.0, precision, 0.2, 0, flags | FLAG_OVERLAP_ITERATIONS) as up:
        up.upload_rgb8(rgb)
        up.execute(4)
        assert np.array_equal(get(up), seq)                              # one stream: nothing to overlap -- the ordered plan, cuts included


def test_four_step_plans_in_a_ring():
    """rows and columns in four steps with frames overlapping on the plan's streams: every lane has its own transposition
    buffer -- three distinct frames through fftup_execute_ring equal the same frames one at a time"""
    from vkresample_amd import synth
    for (W, H, u) in ((9216, 8, 2.0), (16, 4900, 3.0)):       # (16 x 4900 at u = 2 is a one-launch polyphase plan since round 5)
        frames = [synth.frame(90 + k, W, H) for k in range(3)]
        single = []
        with _up(W, H, u, 0) as up:
            for f in frames:
                up.upload_rgb8(f)
                up.execute(1)
                single.append(up.download_planar().copy())
        with _up(W, H, u, 0, ring=3) as up:
            assert "four steps" in up.description
            for s, f in enumerate(frames):
                up.upload_rgb8(f, slot=s)
            up.execute_ring(9, 0)
            for s in range(3):
                assert np.array_equal(up.download_planar(s), single[s])
        assert not np.array_equal(single[0], single[1])


def test_two_pixel_wide_image():
    """uW = 2 (the smallest width the reference's even-size rule admits): the two-launch sharpen computed its grid as uW / 4 / 256
    rounded up -- zero workgroups, a launch error -- until round 5."""
    from vkresample_amd import synth
    rgb = synth.frame(1, 2, 4, "N")
    with _up(2, 4, 1.0, 0, 0.2, 0) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        out = up.download_planar().astype(np.float64)
    _, oout, _ = O.upscale_rgb8(rgb, 1.0, 0, 0.2)
    assert np.abs(out - oout).max() <= 2e-5


@pytest.mark.parametrize("W,H,precision,flags", [(16, 8, 0, 4), (60, 42, 0, 4), (240, 270, 0, 4), (1000, 600, 0, 4), (2048, 1024, 0, 4), (640, 480, 2, 6),
                                                 (16, 8, 1, 0), (60, 42, 1, 0), (240, 270, 1, 0), (1024, 512, 1, 0), (2048, 64, 1, 0), (64, 2048, 1, 0)])
def test_generic_polyphase_column_pass(W, H, precision, flags, monkeypatch):
    """Round 5: size-generic plans with u = 2 run the column pass in polyphase form (k_col_poly: the even rows of the zero-padded
    inverse ARE the rows of S1 over 2 and are never computed; the odd rows are a length-H inverse of the phase-shifted spectrum)
    and the C2R kernel reads the even rows from S1.  Against the full-length form (generic_poly=0 in the test build of the
    library) to rounding, and both against the oracle at the bars of the other tests."""
    from vkresample_amd import _lib, synth
    rgb = synth.frame(21, W, H, "N")
    res = []
    for poly in (1, 0):
        if not poly:
            monkeypatch.setenv("FFTUP_LIBRARY", _lib.KNOBS_LIB_PATH)
            monkeypatch.setenv("FFTUP_EXPERIMENT", "generic_poly=0")
        with _up(W, H, 2.0, precision, 0.2, 0, flags) as up:
            assert ("polyphase" in up.description) == bool(poly), up.description
            up.upload_rgb8(rgb)
            up.execute(2)
            res.append((up.download_presharpen().astype(np.float64), up.download_planar().astype(np.float64)))
    opre, oout, _ = O.upscale_rgb8(rgb, 2.0, precision, 0.2)
    # (-p 2: the pre-sharpen image is binary16 -- one ulp of the value, as the sweeps' bound)
    tol_pre = {0: 2e-6, 1: 1e-12}.get(precision, one_half_ulp_bound(opre))
    for pre, out in res:
        assert (np.abs(pre - opre) <= tol_pre).all()
    assert (np.abs(res[0][0] - res[1][0]) <= tol_pre).all()
    if precision != 2:
        assert np.abs(res[0][1] - oout).max() <= (1e-9 if precision == 1 else 5e-5)
