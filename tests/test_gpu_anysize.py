"""GPU: FFTUP_FLAG_ANY_SIZE (csrc/kernels_bluestein.hpp; Bluestein forward rows: k_row_r2c_odd of csrc/kernels_odd.hpp) -- sizes with
a prime factor above 7 -- against the fp64 statement of the reference's filter at that size:
oracle/ref_layout_emulation.closed_form (quirks B1-B3) followed by oraclelib.sharpen (B4, B5); for FFTUP_FLAG_DOWNSCALE plans
tests/downscale_oracle.py.  The bars are those of tests/paritylib.py; the amplitude-preserving image is sc * R, sc = upsq for an
upscale and (uW uH) / (W H) for a downscale.

Every parity case runs with planar and fused-uint8 input for -p 0 and -p 2, except the two large ones: 1366x768 -u 2 runs -p 0 and
the downscale 2732x1536 -> 1366x768 runs -p 2 in the default run; FFTUP_BIG_TESTS=1 adds the other precision of each."""
import os
import subprocess

import numpy as np
import pytest

import downscale_oracle as S
import oraclelib as O
import paritylib as P
from oracle import ref_layout_emulation as E
from paritylib import CLI
from test_host_anysize import VALID

pytestmark = pytest.mark.gpu
BIG = os.environ.get("FFTUP_BIG_TESTS", "0") != "0"


def _run(W, H, u, precision, flags, rgb=None, planes=None):
    import vkresample_amd as v
    with v.Upscaler(W, H, u, precision, P.SHARPEN, 0, flags | v.FLAG_ANY_SIZE) as up:
        pre, out = P.run_uploaded(up, rgb, planes)
        names, desc = up.kernel_names, up.description
        assert not up.tuned and not up.u8_store
    return pre, out, names, desc


def _check(W, H, u, precision, down, uint8, seed, tag, pooled=None):
    """sc * R is the amplitude-preserving image y: sc = upsq for an upscale, (uW uH) / (W H) for a downscale"""
    import vkresample_amd as v
    rgb, planes, x = P.inputs(W, H, precision, uint8, seed)
    flags = (v.FLAG_DOWNSCALE if down else 0) | (v.FLAG_FUSE_U8_LOAD if uint8 else 0)
    pre, out, names, desc = _run(W, H, u, precision, flags, rgb, planes)
    assert any(n.endswith("_bz") for n in names) and "bluestein L=" in desc, (names, desc)
    if down:
        uW, uH = S.out_size(W, u), S.out_size(H, u)
        R = S.fft_down_R(x, uW, uH)
        sc = uW * uH / (W * H)
    else:
        uW, uH = E.out_dims(W, H, u)
        R = E.closed_form(x, u)
        sc = float(np.float32(u)) ** 2
    assert pre.shape == R.shape == (3, uH, uW)
    P.assert_parity(tag, precision, pre, out, sc * R, sc, u, pooled=pooled)
    return pre, x


# 46x22: Bluestein on all four transforms; 640x482: columns only (482 = 2 * 241); 1000x800 -u 1.1: the inverses only (1100, 880);
# 4094x64 -u 1: L = 8192; 16x262: a thin frame whose Bluestein column pass (524 points through L = 1050, tiles of 8) needs 142 816 bytes
# of dynamic LDS -- above the 64 KB a kernel gets without its attribute
UP = [(46, 22, 2.0), (640, 482, 2.0), (1000, 800, 1.1), (92, 44, 1.5), (1170, 844, 2.0), (4094, 64, 1.0), (16, 262, 2.0)]


@pytest.mark.parametrize("W,H,u", UP)
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("uint8", [False, True])
def test_anysize_parity(W, H, u, precision, uint8):
    pre, x = _check(W, H, u, precision, False, uint8, W + H + precision, "anysize p%d %dx%d u%.4g u8%d" % (precision, W, H, u, uint8))
    if u == 1.0 and precision == 0:
        # -u 1 reproduces the input (the oracle does, to 7e-16): nothing is padded, no Nyquist quirk applies
        P.assert_identity("anysize identity %dx%d" % (W, H), pre, x)


@pytest.mark.parametrize("precision", [0, 2] if BIG else [0])
@pytest.mark.parametrize("uint8", [False, True])
def test_anysize_parity_1366x768(precision, uint8):
    """Bluestein rows (1366, 2732), untouched columns (768, 1536: the polyphase column kernel)"""
    _check(1366, 768, 2.0, precision, False, uint8, 1366 + precision, "anysize p%d 1366x768 u2 u8%d" % (precision, uint8))


DOWN = [(124, 76, 0.5, 0), (124, 76, 0.5, 2), (2732, 1536, 0.5, 2)] + ([(2732, 1536, 0.5, 0)] if BIG else [])


@pytest.mark.parametrize("W,H,u,precision", DOWN)
@pytest.mark.parametrize("uint8", [False, True])
def test_anysize_down_parity(W, H, u, precision, uint8):
    _check(W, H, u, precision, True, uint8, W + H + precision, "anysize_down p%d %dx%d u%.4g u8%d" % (precision, W, H, u, uint8))


@pytest.mark.parametrize("k", [1, 341, 682])
def test_single_cosine_comes_back_resampled(k):
    """what the oracle alone cannot hide: 0.5 + a cos(2 pi k x / W) at 1366 wide comes back as upsq R = 0.5 + a cos(2 pi k x' / uW)
    (k below the Nyquist bin 683; fp64: 3e-13)"""
    W, H, a = 1366, 64, 0.3
    xx = np.arange(W)
    row = 0.5 + a * np.cos(2 * np.pi * k * xx / W)
    x = np.broadcast_to(row, (3, H, W)).astype(np.float32)
    pre, _, _, _ = _run(W, H, 2.0, 0, 0, planes=np.ascontiguousarray(x))
    want = np.broadcast_to(0.5 + a * np.cos(2 * np.pi * k * np.arange(2 * W) / (2 * W)), (3, 2 * H, 2 * W))
    # (the fp32 input's own rounding: compare with the exact resampling of the rounded input as well)
    ref = 4.0 * E.closed_form(x.astype(np.float64), 2.0)
    P.measured("anysize cosine k=%d" % k, max_err=np.abs(4.0 * pre - want).max(), l2=P.rel_l2(4.0 * pre, want), oracle_max=np.abs(ref - want).max())
    assert P.rel_l2(4.0 * pre, want) <= P.FP32_PRE_L2
    assert np.abs(4.0 * pre - want).max() <= P.FP32_PRE_MAX


@pytest.mark.parametrize("W,H,u,down", [(2048, 1024, 2.0, False), (640, 480, 1.5, False), (4096, 2048, 0.5, True)])
def test_flag_is_a_no_op_on_smooth_plans(W, H, u, down):
    import vkresample_amd as v
    rgb = P.frame(W, H, seed=5)
    got = []
    for flags in (0, v.FLAG_ANY_SIZE):
        with v.Upscaler(W, H, u, 0, 0.2, 0, flags | (v.FLAG_DOWNSCALE if down else 0)) as up:
            up.upload_rgb8(rgb)
            up.execute(1)
            got.append((up.download_planar().tobytes(), up.tuned, up.specialised_at_plan_time, up.num_kernels, up.kernel_names, up.description,
                        up.alg_bytes_per_frame, up.device_bytes))
    assert got[0][1:] == got[1][1:], (got[0][1:], got[1][1:])
    assert got[0][0] == got[1][0]


@pytest.mark.parametrize("precision", [0, 2])
def test_every_execution_path_gives_the_same_bytes(precision):
    """a Bluestein plan (1366x768 -u 2): execute against execute_ring slot by slot, submit_rgb8 and submit_png against upload +
    execute + download_rgb8, FLAG_OVERLAP_ITERATIONS against ordered iterations, equal output checksums"""
    import vkresample_amd as v
    W, H, u = 1366, 768, 2.0
    flags = v.FLAG_ANY_SIZE
    frames = [np.ascontiguousarray(P.frame(W, H, seed=60 + k)) for k in range(3)]
    want, planes, sums = [], [], []
    with v.Upscaler(W, H, u, precision, 0.2, 0, flags) as up:
        for f in frames:
            up.upload_rgb8(f)
            up.execute(1)
            want.append(up.download_rgb8())
            planes.append(up.download_planar().tobytes())
            sums.append(up.output_checksum())
        ms = up.profile_kernels(2)
        assert len(ms) >= 4 and all(t > 0 for t in list(ms)[:4])
        uW, uH = up.out_width, up.out_height
    with v.Upscaler(W, H, u, precision, 0.2, 0, flags | v.FLAG_OVERLAP_ITERATIONS) as up:
        up.upload_rgb8(frames[0])
        up.execute(5)
        assert up.download_planar().tobytes() == planes[0]
        assert up.output_checksum() == sums[0]
    with v.Upscaler(W, H, u, precision, 0.2, 0, flags | v.FLAG_FUSE_U8_STORE | v.FLAG_TUNE_PLAN | v.FLAG_UNFUSED_SHARPEN, 3) as up:
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


def test_anysize_cli(tmp_path):
    """-anysize -u 2 on a 1366x768 PNG gives the API's pixels, single-image and batched; without -anysize the CLI refuses with the
    code's own message and names the option"""
    import vkresample_amd as v
    rgb = P.frame(1366, 768, seed=78)
    with v.Upscaler(1366, 768, 2.0, 0, 0.2, 0, v.FLAG_ANY_SIZE) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        want = up.download_rgb8()
    P.png_write(tmp_path / "in.png", rgb)
    r = subprocess.run([CLI, "-anysize", "-i", "in.png", "-o", "out.png", "-u", "2", "-n", "1"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(P.png_read(tmp_path / "out.png"), want)
    r = subprocess.run([CLI, "-i", "in.png", "-o", "bad.png", "-u", "2", "-n", "1"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 2 and not (tmp_path / "bad.png").exists()
    assert "unsupported size" in r.stdout + r.stderr and "-anysize" in r.stdout + r.stderr
    (tmp_path / "inp").mkdir()
    (tmp_path / "outp").mkdir()
    P.png_write(tmp_path / "inp" / "000001.png", rgb)
    r = subprocess.run([CLI, "-ifolder", "inp", "-ofolder", "outp", "-numfiles", "1", "-u", "2", "-anysize"], capture_output=True, text=True,
                       cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(P.png_read(tmp_path / "outp" / "000001.png"), want)


def test_anysize_plan_info_and_errors():
    import vkresample_amd as v
    from vkresample_amd import _lib
    from test_host_anysize import test_invalid_plans_fail_before_device_access as invalid
    with v.Upscaler(1366, 768, 2.0, 0, 0.2, 0, v.FLAG_ANY_SIZE | v.FLAG_GENERIC_KERNELS) as up:
        assert up.kernel_names == ["row_r2c_bz", "col_fwd_pad_inv", "row_c2r_bz", "sharpen"]
        assert "rows 1366->2732 bluestein L=2744/5488" in up.description and "columns" not in up.description.split("bluestein", 1)[1]
        assert up.num_kernels == 4 and not up.tuned and not up.u8_store
    with v.Upscaler(1000, 800, 1.1, 2, 0.2, 0, v.FLAG_ANY_SIZE) as up:
        assert up.kernel_names == ["row_r2c", "col_fwd_pad_inv_bz", "row_c2r_bz", "sharpen"]
        assert "rows 1000->1100 bluestein L=-/" in up.description and "columns 800->880 bluestein L=-/" in up.description
    with v.Upscaler(2732, 1536, 0.5, 0, 0.2, 0, v.FLAG_ANY_SIZE | v.FLAG_DOWNSCALE) as up:
        assert up.kernel_names == ["row_r2c_crop_bz", "col_fwd_crop_inv", "row_c2r_bz", "sharpen"]
    # the same codes as without a device (tests/test_host_anysize.py)
    for W, H, u, extra in VALID:
        with pytest.raises(v.FftupError) as e:
            v.Upscaler(W, H, u, 0, 0.2, 0, v.FLAG_DOWNSCALE if extra == "down" else extra)
        assert e.value.code == 2
    for mark in invalid.pytestmark:
        if mark.name == "parametrize":
            for kwargs, code in mark.args[1]:
                invalid(kwargs, code)
    import ctypes
    desc = ctypes.create_string_buffer(256)
    assert _lib.load().fftup_jit_check(1366, 768, 2.0, 0, b"", desc, 256) == 2
