"""GPU: FFTUP_FLAG_ODD_SIZE (csrc/kernels_odd.hpp) -- plans with an odd width or height, input or output -- against the fp64
statement of exact trigonometric resampling, tests/oddsize_oracle.py, followed by oraclelib.sharpen (quirks B4, B5; B1-B3 do not
apply to these plans), at the bars of tests/paritylib.py.  The amplitude-preserving image is sc * R, sc = uW uH / (W H).

Every parity case runs with planar and fused-uint8 input for -p 0 and -p 2, except the large ones: 1215x675 -u 2 and 1365x767 -u 2
run -p 0 and the downscale 2730x1534 -> 1365x767 runs -p 2 in the default run; FFTUP_BIG_TESTS=1 adds the other precision."""
import os
import subprocess

import numpy as np
import pytest

import oddsize_oracle as Q
import oraclelib as O
import paritylib as P
from paritylib import CLI
from test_host_oddsize import VALID, VALID_ANY

pytestmark = pytest.mark.gpu
BIG = os.environ.get("FFTUP_BIG_TESTS", "0") != "0"
LARGE = {(1215, 675, 2.0): 0, (1365, 767, 2.0): 0, (2730, 1534, 0.5): 2}         # the precision of the default run


def _flags(v, extra):
    return (v.FLAG_DOWNSCALE if "down" in extra else 0) | (v.FLAG_ANY_SIZE if "any" in extra else 0) | v.FLAG_ODD_SIZE


def _run(W, H, u, precision, flags, rgb=None, planes=None):
    import vkresample_amd as v
    with v.Upscaler(W, H, u, precision, P.SHARPEN, 0, flags) as up:
        pre, out = P.run_uploaded(up, rgb, planes)
        names, desc = up.kernel_names, up.description
        assert not up.tuned and not up.u8_store and up.num_kernels == 4
    return pre, out, names, desc


def _check(W, H, u, precision, extra, uint8, seed, tag, pooled=None):
    import vkresample_amd as v
    rgb, planes, x = P.inputs(W, H, precision, uint8, seed)
    pre, out, names, desc = _run(W, H, u, precision, _flags(v, extra) | (v.FLAG_FUSE_U8_LOAD if uint8 else 0), rgb, planes)
    assert all("_odd" in n for n in names[:3]) and names[3] == "sharpen", names
    uW, uH = Q.out_size(W, u), Q.out_size(H, u)
    assert "rows %d->%d" % (W, uW) in desc and "columns %d->%d" % (H, uH) in desc, desc
    R = Q.resample_R(x, uW, uH)
    sc = uW * uH / (W * H)
    assert pre.shape == R.shape == (3, uH, uW)
    P.assert_parity(tag, precision, pre, out, sc * R, sc, u, pooled=pooled)
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
        P.assert_identity("oddsize identity %dx%d" % (W, H), pre, x)


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
    P.measured("oddsize cosine k=%d" % k, max_err=np.abs(4.0 * pre - want).max(), l2=P.rel_l2(4.0 * pre, want), oracle_max=np.abs(ref - want).max())
    assert P.rel_l2(4.0 * pre, want) <= P.FP32_PRE_L2
    assert np.abs(4.0 * pre - want).max() <= P.FP32_PRE_MAX


@pytest.mark.parametrize("W,H,u,extra", [(2048, 1024, 2.0, ""), (640, 480, 1.5, ""), (4096, 2048, 0.5, "down"), (640, 482, 2.0, "any")])
def test_flag_is_a_no_op_on_even_plans(W, H, u, extra):
    import vkresample_amd as v
    rgb = P.frame(W, H, seed=5)
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


@pytest.mark.parametrize("W,H,extra", [(1215, 675, ""), (1365, 767, "any")])
@pytest.mark.parametrize("precision", [0, 2])
def test_every_execution_path_gives_the_same_bytes(W, H, extra, precision):
    """execute against execute_ring slot by slot, submit_rgb8 and submit_png against upload + execute + download_rgb8,
    FLAG_OVERLAP_ITERATIONS against ordered iterations, equal output checksums (and the checksum is the sum of the words)"""
    import vkresample_amd as v
    u = 2.0
    flags = _flags(v, extra)
    frames = [np.ascontiguousarray(P.frame(W, H, seed=60 + k)) for k in range(3)]
    want, planes, sums = [], [], []
    with v.Upscaler(W, H, u, precision, 0.2, 0, flags) as up:
        for f in frames:
            up.upload_rgb8(f)
            up.execute(1)
            want.append(up.download_rgb8())
            planes.append(up.download_planar().tobytes())
            sums.append(up.output_checksum())
            assert sums[-1] == P.word_sum(planes[-1])
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
            assert np.array_equal(P.png_pixels(bytes(buf[:n]), uW, uH), want[k]), k
        # the input tap: what the fused-load row kernel computes on is what the unpack kernel stores
        up.upload_rgb8(frames[1], 0)
        assert np.array_equal(up.download_input_planar(0).astype(np.float64), O.load_lut(precision)[np.transpose(frames[1], (2, 0, 1))])


def test_checksum_of_an_odd_number_of_binary16_pixels():
    """45x21 -u 1 -p 2: 3 * 945 halves = 5670 bytes, two behind the last whole word"""
    import vkresample_amd as v
    with v.Upscaler(45, 21, 1.0, 2, 0.2, 0, v.FLAG_ODD_SIZE) as up:
        up.upload_rgb8(P.frame(45, 21, seed=3))
        up.execute(1)
        b = up.download_planar().tobytes()
        assert len(b) % 4 == 2 and up.output_checksum() == P.word_sum(b)


def test_oddsize_cli(tmp_path):
    """-oddsize -u 2 on a 1215x675 PNG gives the API's pixels, single-image and batched; without -oddsize the CLI exits 1 with the
    code's own message and names the option"""
    import vkresample_amd as v
    rgb = P.frame(1215, 675, seed=78)
    with v.Upscaler(1215, 675, 2.0, 0, 0.2, 0, v.FLAG_ODD_SIZE) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        want = up.download_rgb8()
    P.png_write(tmp_path / "in.png", rgb)
    r = subprocess.run([CLI, "-oddsize", "-i", "in.png", "-o", "out.png", "-u", "2", "-n", "1"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(P.png_read(tmp_path / "out.png"), want)
    r = subprocess.run([CLI, "-i", "in.png", "-o", "bad.png", "-u", "2", "-n", "1"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 1 and not (tmp_path / "bad.png").exists()
    assert "must be even" in r.stdout + r.stderr and "-oddsize" in r.stdout + r.stderr
    (tmp_path / "inp").mkdir()
    (tmp_path / "outp").mkdir()
    P.png_write(tmp_path / "inp" / "000001.png", rgb)
    r = subprocess.run([CLI, "-ifolder", "inp", "-ofolder", "outp", "-numfiles", "1", "-u", "2", "-oddsize"], capture_output=True, text=True,
                       cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(P.png_read(tmp_path / "outp" / "000001.png"), want)


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
