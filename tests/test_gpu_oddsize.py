"""GPU: FFTUP_FLAG_ODD_SIZE (csrc/kernels_odd.hpp) -- plans with an odd width or height, input or output -- against the fp64
statement of exact trigonometric resampling, tests/oddsize_oracle.py, followed by oraclelib.sharpen (quirks B4, B5; B1-B3 do not
apply to these plans).

Bars: the project's, as stated at the top of tests/test_gpu_downscale.py and used by tests/test_gpu_anysize.py.  fp32: the
amplitude-preserving image sc * pre, sc = uW uH / (W H), within relative L2 2e-6 and max 1e-5 of the oracle's y; the sharpened
output against oraclelib.sharpen applied to the oracle's R within relative L2 5e-6 and max 2e-5.  fp16 (-p 2): R within one
binary16 ulp of the oracle's own binary16 value and different from it in <= 1 % of the pixels; output relative L2 <= 3.5e-4,
different in <= 2 %, max 8e-3.  The last output row is compared too: its reads
past the end of a plane, undefined in the reference (quirk B5), are defined here as "same column, last written row"
(oracle/fftup_oracle.c), and the HIP path is held to that definition.

Every parity case runs with planar and fused-uint8 input for -p 0 and -p 2, except the large ones: 1215x675 -u 2 and 1365x767 -u 2
run -p 0 and the downscale 2730x1534 -> 1365x767 runs -p 2 in the default run; FFTUP_BIG_TESTS=1 adds the other precision."""
import os
import subprocess

import numpy as np
import pytest

import oddsize_oracle as Q
import oraclelib as O
from test_gpu_dct import _png_pixels, _png_read, _png_write
from test_host_oddsize import VALID, VALID_ANY

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vkresample_amd", "vkresample")
BIG = os.environ.get("FFTUP_BIG_TESTS", "0") != "0"
LARGE = {(1215, 675, 2.0): 0, (1365, 767, 2.0): 0, (2730, 1534, 0.5): 2}         # the precision of the default run


def _rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30))


def _m(tag, **vals):
    print("MEASURED %s: %s" % (tag, "  ".join("%s %.3g" % kv for kv in vals.items())))


def _frame(W, H, seed=0, dist="N"):
    from vkresample_amd import synth
    return synth.frame(seed, W, H, dist)


def _flags(v, extra):
    return (v.FLAG_DOWNSCALE if "down" in extra else 0) | (v.FLAG_ANY_SIZE if "any" in extra else 0) | v.FLAG_ODD_SIZE


def _inputs(W, H, precision, uint8, seed):
    """(rgb, planes, x) as tests/test_gpu_downscale.py: what is uploaded and the values the plan computes on"""
    rgb = _frame(W, H, seed=seed)
    if uint8:
        return rgb, None, O.load_lut(precision)[np.transpose(rgb, (2, 0, 1))]
    x = np.transpose(rgb, (2, 0, 1)) / 255.0 + np.random.RandomState(seed).rand(3, H, W) / 512.0
    planes = x.astype(np.float16 if precision == 2 else np.float32)
    return None, planes, planes.astype(np.float64)


def _run(W, H, u, precision, flags, rgb=None, planes=None):
    import vkresample_amd as v
    with v.Upscaler(W, H, u, precision, 0.2, 0, flags) as up:
        if rgb is not None:
            up.upload_rgb8(rgb)
        else:
            up.upload_planar(planes)
        up.execute(1)
        pre = up.download_presharpen().astype(np.float64)
        out = up.download_planar().astype(np.float64)
        names, desc = up.kernel_names, up.description
        assert not up.tuned and not up.u8_store and up.num_kernels == 4
    return pre, out, names, desc


def _check(W, H, u, precision, extra, uint8, seed, tag, pooled=None):
    import vkresample_amd as v
    rgb, planes, x = _inputs(W, H, precision, uint8, seed)
    pre, out, names, desc = _run(W, H, u, precision, _flags(v, extra) | (v.FLAG_FUSE_U8_LOAD if uint8 else 0), rgb, planes)
    assert all("_odd" in n for n in names[:3]) and names[3] == "sharpen", names
    uW, uH = Q.out_size(W, u), Q.out_size(H, u)
    assert "rows %d->%d" % (W, uW) in desc and "columns %d->%d" % (H, uH) in desc, desc
    R = Q.resample_R(x, uW, uH)
    sc = uW * uH / (W * H)
    assert pre.shape == R.shape == (3, uH, uW)
    y = sc * R
    if precision == 0:
        sh = O.sharpen(R, u, 0, 0.2)
        _m(tag, pre_l2=_rel_l2(sc * pre, y), pre_max=np.abs(sc * pre - y).max(),
           out_l2=_rel_l2(out, sh), out_max=np.abs(out - sh).max())
        assert _rel_l2(sc * pre, y) <= 2e-6
        assert np.abs(sc * pre - y).max() <= 1e-5
        assert _rel_l2(out, sh) <= 5e-6
        assert np.abs(out - sh).max() <= 2e-5
    else:
        opre = R.astype(np.float16).astype(np.float64)
        ulp = np.maximum(np.abs(opre), 2.0 ** -14) * 2.0 ** -10
        sh = O.sharpen(opre, u, 2, 0.2)
        _m(tag, pre_diff_frac=(pre != opre).mean(), pre_max_ulps=(np.abs(pre - opre) / ulp).max(),
           out_l2=_rel_l2(out, sh), out_max=np.abs(out - sh).max(),
           out_diff_frac=(out != sh).mean())
        assert (np.abs(pre - opre) <= ulp * 1.0001 + 5e-7).all()
        assert _rel_l2(out, sh) <= 3.5e-4
        assert np.abs(out - sh).max() <= 8e-3
        if pooled is None:
            assert (pre != opre).mean() <= 0.01
            assert (out != sh).mean() <= 0.02
        else:                                   # (an output of a few dozen values: the two fractions are asserted on the pooled counts)
            pooled.append((int((pre != opre).sum()), pre.size, int((out != sh).sum()), out.size))
    return pre, x


def _precisions(W, H, u):
    p = LARGE.get((W, H, u))
    return [0, 2] if p is None or BIG else [p]


# 105x63 -u 1: the identity on smooth odd lengths; 90x45 -u 1.5 (135x67): the only odd length is H ... and uH; 64x45 -u 2: H only;
# 50x32 -u 1.5 (75x48): uW only
EXTRA = [(105, 63, 1.0, "", None), (64, 45, 2.0, "", None), (50, 32, 1.5, "", None)]
# 15x243 -u 2: a thin frame whose column pass (486 points, tiles of 8) needs 66 112 bytes of dynamic LDS -- above the 64 KB a kernel
# gets without its attribute
THIN = [(15, 243, 2.0, "", None)]
CASES = [(W, H, u, extra, p, u8) for (W, H, u, extra, _) in VALID + VALID_ANY + EXTRA + THIN for p in _precisions(W, H, u) for u8 in (False, True)]


@pytest.mark.parametrize("W,H,u,extra,precision,uint8", CASES)
def test_oddsize_parity(W, H, u, extra, precision, uint8):
    pre, x = _check(W, H, u, precision, extra, uint8, W + H + precision, "oddsize p%d %dx%d u%.4g %s u8%d" % (precision, W, H, u, extra, uint8))
    if u == 1.0 and precision == 0:
        # -u 1 reproduces the input (the oracle does, to 6e-16)
        _m("oddsize identity %dx%d" % (W, H), max_err=np.abs(pre - x).max(), l2=_rel_l2(pre, x))
        assert _rel_l2(pre, x) <= 2e-6 and np.abs(pre - x).max() <= 1e-5


def test_only_odd_length_is_h_or_uw():
    """the two EXTRA plans with one odd length: which one it is"""
    assert (Q.out_size(64, 2.0), Q.out_size(45, 2.0)) == (128, 90) and (Q.out_size(50, 1.5), Q.out_size(32, 1.5)) == (75, 48)


@pytest.mark.parametrize("k", [1, 341, 682])
def test_single_cosine_comes_back_resampled(k):
    """what the oracle alone cannot hide: 0.5 + a cos(2 pi k x / W) at 1365 wide comes back as sc R = 0.5 + a cos(2 pi k x' / uW)
    (k below W/2 = 682.5: an odd length has no Nyquist bin)"""
    import vkresample_amd as v
    W, H, a = 1365, 63, 0.3
    row = 0.5 + a * np.cos(2 * np.pi * k * np.arange(W) / W)
    x = np.ascontiguousarray(np.broadcast_to(row, (3, H, W)).astype(np.float32))
    pre, _, _, _ = _run(W, H, 2.0, 0, v.FLAG_ODD_SIZE | v.FLAG_ANY_SIZE, planes=x)
    want = np.broadcast_to(0.5 + a * np.cos(2 * np.pi * k * np.arange(2 * W) / (2 * W)), (3, 2 * H, 2 * W))
    # (the fp32 input's own rounding: the exact resampling of the rounded input as well)
    ref = 4.0 * Q.resample_R(x.astype(np.float64), 2 * W, 2 * H)
    _m("oddsize cosine k=%d" % k, max_err=np.abs(4.0 * pre - want).max(), l2=_rel_l2(4.0 * pre, want), oracle_max=np.abs(ref - want).max())
    assert _rel_l2(4.0 * pre, want) <= 2e-6
    assert np.abs(4.0 * pre - want).max() <= 1e-5


@pytest.mark.parametrize("W,H,u,extra", [(2048, 1024, 2.0, ""), (640, 480, 1.5, ""), (4096, 2048, 0.5, "down"), (640, 482, 2.0, "any")])
def test_flag_is_a_no_op_on_even_plans(W, H, u, extra):
    import vkresample_amd as v
    rgb = _frame(W, H, seed=5)
    base = _flags(v, extra) & ~v.FLAG_ODD_SIZE
    got = []
    for flags in (base, base | v.FLAG_ODD_SIZE):
        with v.Upscaler(W, H, u, 0, 0.2, 0, flags) as up:
            up.upload_rgb8(rgb)
            up.execute(1)
            got.append((up.download_planar().tobytes(), up.tuned, up.specialised_at_plan_time, up.num_kernels, up.kernel_names, up.description,
                        up.alg_bytes_per_frame, up.kernel_alg_bytes, up.kernel_min_bytes, up.device_bytes, up.output_checksum()))
    assert got[0][1:] == got[1][1:], (got[0][1:], got[1][1:])
    assert got[0][0] == got[1][0]


def _word_sum(b):
    """fftup_output_checksum in numpy: the 32-bit little-endian words, the bytes behind the last whole word as one more"""
    b = b + b"\0" * (-len(b) % 4)
    return int(np.frombuffer(b, "<u4").astype(np.uint64).sum() & np.uint64(0xFFFFFFFFFFFFFFFF))


@pytest.mark.parametrize("W,H,extra", [(1215, 675, ""), (1365, 767, "any")])
@pytest.mark.parametrize("precision", [0, 2])
def test_every_execution_path_gives_the_same_bytes(W, H, extra, precision):
    """execute against execute_ring slot by slot, submit_rgb8 and submit_png against upload + execute + download_rgb8,
    FLAG_OVERLAP_ITERATIONS against ordered iterations, equal output checksums (and the checksum is the sum of the words)"""
    import vkresample_amd as v
    u = 2.0
    flags = _flags(v, extra)
    frames = [np.ascontiguousarray(_frame(W, H, seed=60 + k)) for k in range(3)]
    want, planes, sums = [], [], []
    with v.Upscaler(W, H, u, precision, 0.2, 0, flags) as up:
        for f in frames:
            up.upload_rgb8(f)
            up.execute(1)
            want.append(up.download_rgb8())
            planes.append(up.download_planar().tobytes())
            sums.append(up.output_checksum())
            assert sums[-1] == _word_sum(planes[-1])
        ms = up.profile_kernels(2)
        assert len(ms) >= 4 and all(t > 0 for t in list(ms)[:4])
        uW, uH = up.out_width, up.out_height
    with v.Upscaler(W, H, u, precision, 0.2, 0, flags | v.FLAG_OVERLAP_ITERATIONS) as up:
        up.upload_rgb8(frames[0])
        up.execute(5)
        assert up.download_planar().tobytes() == planes[0]
        assert up.output_checksum() == sums[0]
    with v.Upscaler(W, H, u, precision, 0.2, 0, flags | v.FLAG_FUSE_U8_STORE | v.FLAG_TUNE_PLAN | v.FLAG_UNFUSED_SHARPEN | v.FLAG_GENERIC_KERNELS, 3) as up:
        assert not up.u8_store and not up.tuned
        for s, f in enumerate(frames):
            up.upload_rgb8(f, s)
        up.execute_ring(3)
        for s in range(3):
            assert up.download_planar(s).tobytes() == planes[s], s
            assert np.array_equal(up.download_rgb8(s), want[s]), s
            assert up.output_checksum(s) == sums[s], s
        up.execute_ring_timed(3)
        assert up.download_planar(1).tobytes() == planes[1]
        out = np.empty((uH, uW, 3), np.uint8)
        for k in (1, 2, 0):
            up.wait(up.submit_rgb8(frames[k], out))
            assert np.array_equal(out, want[k]), k
        buf = np.empty(up.png_bound(), np.uint8)
        for k in (2, 0):
            n = up.wait_png(up.submit_png(frames[k]), buf)
            assert np.array_equal(_png_pixels(bytes(buf[:n]), uW, uH), want[k]), k
        # the input tap: what the fused-load row kernel computes on is what the unpack kernel stores
        up.upload_rgb8(frames[1], 0)
        assert np.array_equal(up.download_input_planar(0).astype(np.float64), O.load_lut(precision)[np.transpose(frames[1], (2, 0, 1))])


def test_checksum_of_an_odd_number_of_binary16_pixels():
    """45x21 -u 1 -p 2: 3 * 945 halves = 5670 bytes, two behind the last whole word"""
    import vkresample_amd as v
    with v.Upscaler(45, 21, 1.0, 2, 0.2, 0, v.FLAG_ODD_SIZE) as up:
        up.upload_rgb8(_frame(45, 21, seed=3))
        up.execute(1)
        b = up.download_planar().tobytes()
        assert len(b) % 4 == 2 and up.output_checksum() == _word_sum(b)


def test_oddsize_cli(tmp_path):
    """-oddsize -u 2 on a 1215x675 PNG gives the API's pixels, single-image and batched; without -oddsize the CLI exits 1 with the
    code's own message and names the option"""
    import vkresample_amd as v
    rgb = _frame(1215, 675, seed=78)
    with v.Upscaler(1215, 675, 2.0, 0, 0.2, 0, v.FLAG_ODD_SIZE) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        want = up.download_rgb8()
    _png_write(tmp_path / "in.png", rgb)
    r = subprocess.run([CLI, "-oddsize", "-i", "in.png", "-o", "out.png", "-u", "2", "-n", "1"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(_png_read(tmp_path / "out.png"), want)
    r = subprocess.run([CLI, "-i", "in.png", "-o", "bad.png", "-u", "2", "-n", "1"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 1 and not (tmp_path / "bad.png").exists()
    assert "must be even" in r.stdout + r.stderr and "-oddsize" in r.stdout + r.stderr
    (tmp_path / "inp").mkdir()
    (tmp_path / "outp").mkdir()
    _png_write(tmp_path / "inp" / "000001.png", rgb)
    r = subprocess.run([CLI, "-ifolder", "inp", "-ofolder", "outp", "-numfiles", "1", "-u", "2", "-oddsize"], capture_output=True, text=True,
                       cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(_png_read(tmp_path / "outp" / "000001.png"), want)


def test_oddsize_plan_info_and_errors():
    import vkresample_amd as v
    from test_host_oddsize import test_invalid_plans_fail_before_device_access as invalid
    with v.Upscaler(1215, 675, 2.0, 0, 0.2, 0, v.FLAG_ODD_SIZE | v.FLAG_GENERIC_KERNELS) as up:
        assert up.kernel_names == ["row_r2c_odd", "col_fwd_pad_inv_odd", "row_c2r_odd", "sharpen"]
        assert "bluestein" not in up.description
        assert up.num_kernels == 4 and not up.tuned and not up.u8_store
    with v.Upscaler(1365, 767, 2.0, 2, 0.2, 0, v.FLAG_ODD_SIZE | v.FLAG_ANY_SIZE) as up:
        assert up.kernel_names == ["row_r2c_odd_bz", "col_fwd_pad_inv_odd_bz", "row_c2r_odd_bz", "sharpen"]
        assert "rows 1365->2730 bluestein L=2744/5488" in up.description and "columns 767->1534 bluestein L=1536/3072" in up.description
    with v.Upscaler(4095, 63, 1.0, 0, 0.2, 0, v.FLAG_ODD_SIZE | v.FLAG_ANY_SIZE) as up:
        assert "bluestein L=8192/8192" in up.description
    with v.Upscaler(125, 75, 0.6, 0, 0.2, 0, v.FLAG_ODD_SIZE | v.FLAG_DOWNSCALE) as up:
        assert up.kernel_names == ["row_r2c_crop_odd", "col_fwd_crop_inv_odd", "row_c2r_odd", "sharpen"]
    # the same codes as without a device (tests/test_host_oddsize.py)
    for W, H, u, extra, _ in VALID + VALID_ANY:
        with pytest.raises(v.FftupError) as e:
            v.Upscaler(W, H, u, 0, 0.2, 0, _flags(v, extra) & ~v.FLAG_ODD_SIZE)
        assert e.value.code == 1
    for mark in invalid.pytestmark:
        if mark.name == "parametrize":
            for kwargs, code in mark.args[1]:
                invalid(kwargs, code)
