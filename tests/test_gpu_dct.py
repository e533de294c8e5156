"""GPU: the DCT upscale mode (FFTUP_FLAG_DCT, csrc/kernels_dct.hpp) against the fp64 matrix oracle of tests/dct_oracle.py, followed by
oraclelib.sharpen, at the bars of tests/paritylib.py.  The amplitude-preserving image is y = upsq R, upsq as the plan holds it: at
-p 2 rounded to binary16 (dct_oracle.upsq(u, half)).  The input is always an 8-bit frame.
"""
import subprocess

import numpy as np
import pytest

import dct_oracle as D
import oraclelib as O
import paritylib as P
from paritylib import CLI

pytestmark = pytest.mark.gpu


def _run(rgb, u, precision, flags=0):
    import vkresample_amd as v
    H, W, _ = rgb.shape
    with v.Upscaler(W, H, u, precision, P.SHARPEN, 0, flags | v.FLAG_DCT) as up:
        return P.run_uploaded(up, rgb)


# (the 3*5*7 size: 840 = 2^3 3 5 7, 336 = 2^4 3 7 -- 1050 x 420 at -u 1.25, 2520 x 1008 at -u 3)
# 16x256 -u 2: a thin frame whose column pass (512 points, tiles of 8) needs 69 648 bytes of dynamic LDS -- above the 64 KB a kernel
# gets without its attribute, for both input kinds (fuse)
SIZES_FP32 = [(64, 32, 2.0), (96, 60, 1.5), (640, 480, 2.0), (1920, 1080, 2.0), (840, 336, 1.25), (840, 336, 3.0), (16, 256, 2.0)]


def _check(W, H, u, precision, fuse, seed, tag, pooled=None):
    """one plan against the oracle; `pooled`: see paritylib.assert_parity (tests/test_gpu_family_sweep.py)"""
    import vkresample_amd as v
    rgb = P.frame(W, H, seed=seed)
    pre, out = _run(rgb, u, precision, v.FLAG_FUSE_U8_LOAD if fuse else 0)
    x = O.load_lut(precision)[np.transpose(rgb, (2, 0, 1))]
    y = D.resample_planes(x, D.out_size(W, u), D.out_size(H, u))
    assert pre.shape == y.shape
    P.assert_parity(tag, precision, pre, out, y, D.upsq(u, precision == 2), u, pooled=pooled)
    return pre, rgb


@pytest.mark.parametrize("W,H,u", SIZES_FP32)
@pytest.mark.parametrize("fuse", [False, True])
def test_dct_fp32_parity(W, H, u, fuse):
    _check(W, H, u, 0, fuse, W + H, "dct_fp32 %dx%d u%g fuse%d" % (W, H, u, fuse))


SIZES_FP16 = [(64, 32, 2.0), (96, 60, 1.5), (640, 480, 2.0)]


@pytest.mark.parametrize("W,H,u", SIZES_FP16)
@pytest.mark.parametrize("fuse", [False, True])
def test_dct_fp16_parity(W, H, u, fuse):
    _check(W, H, u, 2, fuse, 3 * W + H, "dct_fp16 %dx%d u%g fuse%d" % (W, H, u, fuse))


def test_dct_ramp_has_no_border_ringing():
    """a 2-D ramp: the DCT plan follows it (at the pixel centres) over the whole frame, the FFT plan wraps at the borders"""
    import vkresample_amd as v
    W, H, u = 128, 64, 2.0
    uW, uH = 256, 128
    yy, xx = np.mgrid[0:H, 0:W]
    planes = np.repeat((0.5 * xx / (W - 1) + 0.5 * yy / (H - 1))[None], 3, axis=0).astype(np.float32)
    errs = {}
    for name, flags in (("dct", v.FLAG_DCT), ("fft", 0)):
        with v.Upscaler(W, H, u, 0, 0.2, 0, flags) as up:
            up.upload_planar(planes)
            up.execute(1)
            y = up.download_presharpen().astype(np.float64) * D.upsq(u)
        if name == "dct":
            px, py = D.centre_positions(W, uW), D.centre_positions(H, uH)
        else:
            px, py = np.arange(uW) * W / uW, np.arange(uH) * H / uH
        ramp = 0.5 * px[None, :] / (W - 1) + 0.5 * py[:, None] / (H - 1)
        errs[name] = np.abs(y - ramp[None]).max()
    P.measured("dct_ramp 128x64 u2", dct_max_err=errs["dct"], fft_max_err=errs["fft"])
    assert errs["dct"] <= 5e-3
    assert errs["fft"] > 0.1


@pytest.mark.parametrize("W,H,u,precision", [(96, 60, 1.5, 0), (128, 64, 2.0, 2)])
def test_dct_paths_give_identical_bytes(W, H, u, precision):
    """submit_rgb8, submit_png, OVERLAP_ITERATIONS and a ring of 4 compute the bytes of blocking upload / execute / download_rgb8"""
    import vkresample_amd as v
    frames = [np.ascontiguousarray(P.frame(W, H, seed=40 + k)) for k in range(4)]
    want = []
    with v.Upscaler(W, H, u, precision, 0.2, 0, v.FLAG_DCT) as up:
        for f in frames:
            up.upload_rgb8(f)
            up.execute(1)
            want.append(up.download_rgb8())
        uW, uH = up.out_width, up.out_height
    with v.Upscaler(W, H, u, precision, 0.2, 0, v.FLAG_DCT | v.FLAG_OVERLAP_ITERATIONS) as up:
        up.upload_rgb8(frames[0])
        up.execute(7)
        assert np.array_equal(up.download_rgb8(), want[0])
    with v.Upscaler(W, H, u, precision, 0.2, 0, v.FLAG_DCT, 4) as up:
        for s, f in enumerate(frames):
            up.upload_rgb8(f, s)
        up.execute_ring(4)
        for s in range(4):
            assert np.array_equal(up.download_rgb8(s), want[s]), s
        out = np.empty((uH, uW, 3), np.uint8)
        for k in (1, 2, 3, 0):
            up.wait(up.submit_rgb8(frames[k], out))
            assert np.array_equal(out, want[k]), k
        buf = np.empty(up.png_bound(), np.uint8)
        for k in (2, 0):
            n = up.wait_png(up.submit_png(frames[k]), buf)
            assert np.array_equal(P.png_pixels(bytes(buf[:n]), uW, uH), want[k]), k


def test_dct_plan_info_and_errors():
    import vkresample_amd as v
    from vkresample_amd import _lib
    assert _lib.load().fftup_version().startswith(b"fftup 0.7.0")
    with v.Upscaler(96, 60, 1.5, 0, 0.2, 0, v.FLAG_DCT | v.FLAG_FUSE_U8_STORE) as up:
        assert up.description.startswith("dct")
        assert up.kernel_names == ["dct_row", "dct_col_pad_idct", "idct_row", "sharpen"]
        assert (up.out_width, up.out_height) == (144, 90)
        assert not up.tuned and not up.u8_store
        C = 3.0
        want = C * 96 * 60 * 4 + 2 * C * 96 * 60 * 4 + 2 * C * 96 * 90 * 4 + 2 * C * 144 * 90 * 4 + C * 144 * 90 * 4
        assert up.alg_bytes_per_frame == pytest.approx(want)
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(64, 32, 2.0, 1, 0.2, 0, v.FLAG_DCT)
    assert e.value.code == 3
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(4200, 64, 2.0, 0, 0.2, 0, v.FLAG_DCT)       # uW = 8400 > 8192 (the FFT plan takes the non-R2C path there)
    assert e.value.code == 2


def test_dct_cli(tmp_path):
    """-dct gives the API's bytes, single-image and batched (-gpupng) mode, and not the FFT's"""
    import vkresample_amd as v
    rgb = P.frame(160, 96, seed=77)
    with v.Upscaler(160, 96, 2.0, 0, 0.2, 0, v.FLAG_DCT) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        want = up.download_rgb8()
    P.png_write(tmp_path / "in.png", rgb)
    outs = {}
    for tag, extra in (("dct", ["-dct"]), ("fft", [])):
        r = subprocess.run([CLI, "-i", "in.png", "-o", tag + ".png", "-u", "2", "-n", "1"] + extra, capture_output=True, text=True,
                           cwd=tmp_path, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = P.png_read(tmp_path / (tag + ".png"))
    assert np.array_equal(outs["dct"], want)
    assert not np.array_equal(outs["fft"], want)
    (tmp_path / "inp").mkdir()
    (tmp_path / "outp").mkdir()
    P.png_write(tmp_path / "inp" / "000001.png", rgb)
    r = subprocess.run([CLI, "-ifolder", "inp", "-ofolder", "outp", "-numfiles", "1", "-u", "2", "-dct", "-gpupng"], capture_output=True,
                       text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(P.png_read(tmp_path / "outp" / "000001.png"), want)


def test_dct_time_against_generic_fft():
    """2048x1024 -> 4096x2048 fp32: the DCT frame against the size-generic FFT frame, ordered iterations, alternating, device events"""
    import vkresample_amd as v
    W, H = 2048, 1024
    rgb = P.frame(W, H, seed=5)
    with v.Upscaler(W, H, 2.0, 0, 0.2, 0, v.FLAG_DCT) as dct, v.Upscaler(W, H, 2.0, 0, 0.2, 0, v.FLAG_GENERIC_KERNELS) as fft:
        dct.upload_rgb8(rgb)
        fft.upload_rgb8(rgb)
        dct.execute(10)
        fft.execute(10)
        td, tf = [], []
        for _ in range(5):
            td.append(dct.execute(20))
            tf.append(fft.execute(20))
        kd = dct.profile_kernels(20)
    d, f = float(np.median(td)), float(np.median(tf))
    P.measured("dct_time 2048x1024 u2 fp32", dct_us=d * 1e3, fft_generic_us=f * 1e3, ratio=d / f,
               dct_row_us=kd[0] * 1e3, dct_col_us=kd[1] * 1e3, idct_row_us=kd[2] * 1e3, sharpen_us=kd[3] * 1e3)
    assert d <= 2.0 * f
