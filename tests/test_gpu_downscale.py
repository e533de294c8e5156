"""GPU: the downscale mode (FFTUP_FLAG_DOWNSCALE, csrc/kernels_downscale.hpp; with FFTUP_FLAG_DCT csrc/kernels_dct.hpp) against
the fp64 oracle of tests/downscale_oracle.py, followed by oraclelib.sharpen, at the bars of tests/paritylib.py.
FFT mode: y = R (uW uH) / (W H); DCT mode: y = upsq R.
"""
import subprocess

import numpy as np
import pytest

import downscale_oracle as S
import paritylib as P
from paritylib import CLI

pytestmark = pytest.mark.gpu


def _scale(W, H, u, dct, half=False):
    """y = scale * R (DCT mode: upsq as the plan holds it -- at -p 2 rounded to binary16, as in tests/test_gpu_dct.py; 0.5^2 and
    0.75^2 are binary16 numbers, 0.4^2 is not)"""
    if dct:
        return S.upsq(u, half)
    return S.out_size(W, u) * S.out_size(H, u) / (W * H)


def _run(W, H, u, precision, flags, rgb=None, planes=None):
    import vkresample_amd as v
    with v.Upscaler(W, H, u, precision, P.SHARPEN, 0, flags | v.FLAG_DOWNSCALE) as up:
        return P.run_uploaded(up, rgb, planes)


def _check(W, H, u, precision, dct, uint8, seed, tag, pooled=None):
    import vkresample_amd as v
    rgb, planes, x = P.inputs(W, H, precision, uint8, seed)
    flags = (v.FLAG_DCT if dct else 0) | (v.FLAG_FUSE_U8_LOAD if uint8 else 0)
    pre, out = _run(W, H, u, precision, flags, rgb, planes)
    uW, uH = S.out_size(W, u), S.out_size(H, u)
    y = S.dct_down_planes(x, uW, uH) if dct else S.fft_down_planes(x, uW, uH)
    assert pre.shape == y.shape == (3, uH, uW)
    P.assert_parity(tag, precision, pre, out, y, _scale(W, H, u, dct, precision == 2), u, pooled=pooled)


# 16x512 -u 0.5: a thin frame whose column pass (512 points, tiles of 8) needs 69 648 bytes of dynamic LDS -- above the 64 KB a
# kernel gets without its attribute
SIZES = [(4096, 2048, 0.5), (2560, 1440, 0.75), (1920, 1080, 2 / 3), (840, 336, 0.5), (2048, 1024, 0.125), (1000, 800, 0.8), (16, 512, 0.5)]


@pytest.mark.parametrize("W,H,u", SIZES)
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("uint8", [False, True])
def test_fft_down_parity(W, H, u, precision, uint8):
    _check(W, H, u, precision, False, uint8, W + H + precision, "down_fft p%d %dx%d u%.4g u8%d" % (precision, W, H, u, uint8))


def test_fft_down_parity_8k():
    _check(7680, 4320, 0.5, 0, False, True, 11, "down_fft p0 7680x4320 u0.5 u8")


# 90x70 -u 0.8: found by tests/test_gpu_family_sweep.py -- a factor whose upsq = "%f"(u u) is no binary16 number: at -p 2 the plan
# divides by the rounded constant (R = y / upsq, the constant of the sharpen pass), and _scale above has to as well
SIZES_DCT = [(96, 60, 0.5), (640, 480, 0.75), (1920, 1080, 0.5), (90, 70, 0.8)]


@pytest.mark.parametrize("W,H,u", SIZES_DCT)
@pytest.mark.parametrize("precision", [0, 2])
def test_dct_down_parity(W, H, u, precision):
    _check(W, H, u, precision, True, precision == 0, 3 * W + H, "down_dct p%d %dx%d u%.4g" % (precision, W, H, u))


def _pre_y(W, H, u, planes, flags=0):
    pre, _ = _run(W, H, u, 0, flags, planes=planes.astype(np.float32))
    return pre * _scale(W, H, u, bool(flags & 256))


def test_constant_frame_stays_constant():
    import vkresample_amd as v
    for flags in (0, v.FLAG_DCT):
        y = _pre_y(1000, 800, 0.8, np.full((3, 800, 1000), 0.37), flags)
        P.measured("down_const flags%d" % flags, max_err=np.abs(y - 0.37).max())
        assert np.abs(y - 0.37).max() <= P.FP32_PRE_MAX


def test_band_limited_frame_decimates():
    """no energy at or above the new Nyquist frequency: the output is x[::d, ::d]"""
    H, W = 256, 512
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.RandomState(1)
    for d in (2, 4):
        x = np.full((3, H, W), 0.5)
        for _ in range(10):
            ky = rng.randint(-(H // d) // 2 + 1, (H // d) // 2)
            kx = rng.randint(-(W // d) // 2 + 1, (W // d) // 2)
            x += 0.04 * np.cos(2 * np.pi * (ky * yy / H + kx * xx / W) + rng.rand() * 6.28)
        x = x.astype(np.float32).astype(np.float64)
        y = _pre_y(W, H, 1.0 / d, x)
        P.measured("down_bandlimited d%d" % d, max_err=np.abs(y - x[:, ::d, ::d]).max())
        assert np.abs(y - x[:, ::d, ::d]).max() <= P.FP32_PRE_MAX


def test_content_above_new_nyquist_vanishes():
    """a cosine at 0.375 cycles per pixel along both axes leaves the mean at u = 1/2 (no aliasing)"""
    H, W = 128, 256
    yy, xx = np.mgrid[0:H, 0:W]
    x = 0.5 + 0.2 * np.cos(2 * np.pi * 0.375 * xx + 0.3) + 0.2 * np.cos(2 * np.pi * 0.375 * yy + 1.1)
    y = _pre_y(W, H, 0.5, np.broadcast_to(x, (3, H, W)))
    P.measured("down_antialias", max_err=np.abs(y - 0.5).max())
    assert np.abs(y - 0.5).max() <= P.FP32_PRE_MAX


def test_fft_up_then_down_returns_the_frame():
    """FFT x2, then upsq R uploaded planar, then the downscale x0.5: x again for frames without energy in the Nyquist row or
    column (the upscale path doubles the Nyquist column, quirk B1)"""
    import vkresample_amd as v
    H, W = 192, 320
    x = np.random.RandomState(2).rand(3, H, W)
    X = np.fft.fft2(x)
    X[:, H // 2, :] = 0
    X[:, :, W // 2] = 0
    x = np.real(np.fft.ifft2(X)).astype(np.float32)
    with v.Upscaler(W, H, 2.0, 0, 0.2, 0, v.FLAG_GENERIC_KERNELS) as up:
        up.upload_planar(x)
        up.execute(1)
        yup = up.download_presharpen() * np.float32(S.upsq(2.0))
    y = _pre_y(2 * W, 2 * H, 0.5, yup)
    P.measured("down_fft_roundtrip", max_err=np.abs(y - x).max())
    assert np.abs(y - x).max() <= P.FP32_PRE_MAX


def test_dct_up_then_down_returns_the_frame():
    import vkresample_amd as v
    H, W = 150, 210
    x = np.random.RandomState(4).rand(3, H, W).astype(np.float32)
    with v.Upscaler(W, H, 2.0, 0, 0.2, 0, v.FLAG_DCT) as up:
        up.upload_planar(x)
        up.execute(1)
        yup = up.download_presharpen() * np.float32(S.upsq(2.0))
    y = _pre_y(2 * W, 2 * H, 0.5, yup, v.FLAG_DCT)
    P.measured("down_dct_roundtrip", max_err=np.abs(y - x).max())
    assert np.abs(y - x).max() <= P.FP32_PRE_MAX


@pytest.mark.parametrize("W,H,u,precision,flags", [(192, 120, 0.5, 0, 0), (256, 128, 0.75, 2, 0), (160, 96, 0.5, 0, 256)])
def test_down_paths_give_identical_bytes(W, H, u, precision, flags):
    """a ring of 4, OVERLAP_ITERATIONS, submit_rgb8 and submit_png compute the bytes of blocking upload / execute / download_rgb8,
    with equal output checksums"""
    import vkresample_amd as v
    flags |= v.FLAG_DOWNSCALE
    frames = [np.ascontiguousarray(P.frame(W, H, seed=60 + k)) for k in range(4)]
    want, sums = [], []
    with v.Upscaler(W, H, u, precision, 0.2, 0, flags) as up:
        for f in frames:
            up.upload_rgb8(f)
            up.execute(1)
            want.append(up.download_rgb8())
            sums.append(up.output_checksum())
        uW, uH = up.out_width, up.out_height
    with v.Upscaler(W, H, u, precision, 0.2, 0, flags | v.FLAG_OVERLAP_ITERATIONS) as up:
        up.upload_rgb8(frames[0])
        up.execute(7)
        assert np.array_equal(up.download_rgb8(), want[0])
        assert up.output_checksum() == sums[0]
    with v.Upscaler(W, H, u, precision, 0.2, 0, flags, 4) as up:
        for s, f in enumerate(frames):
            up.upload_rgb8(f, s)
        up.execute_ring(4)
        for s in range(4):
            assert np.array_equal(up.download_rgb8(s), want[s]), s
            assert up.output_checksum(s) == sums[s], s
        out = np.empty((uH, uW, 3), np.uint8)
        for k in (1, 2, 3, 0):
            up.wait(up.submit_rgb8(frames[k], out))
            assert np.array_equal(out, want[k]), k
        buf = np.empty(up.png_bound(), np.uint8)
        for k in (2, 0):
            n = up.wait_png(up.submit_png(frames[k]), buf)
            assert np.array_equal(P.png_pixels(bytes(buf[:n]), uW, uH), want[k]), k


def test_down_cli(tmp_path):
    """-u 1/2 -downscale gives the API's bytes, single-image and batched (-gpupng); without -downscale the CLI refuses"""
    import vkresample_amd as v
    rgb = P.frame(320, 192, seed=78)
    with v.Upscaler(320, 192, 0.5, 0, 0.2, 0, v.FLAG_DOWNSCALE) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        want = up.download_rgb8()
    P.png_write(tmp_path / "in.png", rgb)
    r = subprocess.run([CLI, "-i", "in.png", "-o", "down.png", "-u", "1/2", "-n", "1", "-downscale"], capture_output=True, text=True,
                       cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(P.png_read(tmp_path / "down.png"), want)
    r = subprocess.run([CLI, "-i", "in.png", "-o", "bad.png", "-u", "0.5", "-n", "1"], capture_output=True, text=True,
                       cwd=tmp_path, timeout=120)
    assert r.returncode != 0 and not (tmp_path / "bad.png").exists()
    (tmp_path / "inp").mkdir()
    (tmp_path / "outp").mkdir()
    P.png_write(tmp_path / "inp" / "000001.png", rgb)
    r = subprocess.run([CLI, "-ifolder", "inp", "-ofolder", "outp", "-numfiles", "1", "-u", "1/2", "-downscale", "-gpupng"],
                       capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(P.png_read(tmp_path / "outp" / "000001.png"), want)


def test_down_plan_info_and_errors():
    import vkresample_amd as v
    from vkresample_amd import _lib
    assert _lib.load().fftup_version().startswith(b"fftup 0.")
    flags = v.FLAG_DOWNSCALE | v.FLAG_FUSE_U8_STORE | v.FLAG_GENERIC_KERNELS | v.FLAG_UNFUSED_SHARPEN | v.FLAG_TUNE_PLAN
    with v.Upscaler(4096, 2048, 0.5, 0, 0.2, 0, flags) as up:
        assert up.description.startswith("downscale:")
        assert up.kernel_names == ["row_r2c_crop", "col_fwd_crop_inv", "row_c2r", "sharpen"]
        assert (up.out_width, up.out_height) == (2048, 1024)
        assert not up.tuned and not up.u8_store
        C, W, H, uW, uH = 3.0, 4096, 2048, 2048, 1024
        inp, S1, S2, R = C * W * H * 4, C * (uW // 2 + 1) * H * 8, C * (uW // 2 + 1) * uH * 8, C * uW * uH * 4
        assert up.alg_bytes_per_frame == pytest.approx(inp + 2 * S1 + 2 * S2 + 2 * R + R)
        assert up.kernel_alg_bytes == pytest.approx([inp + S1, S1 + S2, S2 + R, 2 * R])
        assert up.kernel_min_bytes == pytest.approx(up.kernel_alg_bytes)
    with v.Upscaler(640, 480, 0.75, 2, 0.2, 0, v.FLAG_DOWNSCALE | v.FLAG_DCT) as up:
        assert up.description.startswith("downscale:")
        assert up.kernel_names == ["dct_row", "dct_col_crop_idct", "idct_row", "sharpen"]
        assert (up.out_width, up.out_height) == (480, 360)
        C = 3.0
        want = C * 640 * 480 * 2 + 2 * C * 640 * 480 * 4 + 2 * C * 640 * 360 * 4 + 2 * C * 480 * 360 * 2 + C * 480 * 360 * 2
        assert up.alg_bytes_per_frame == pytest.approx(want)
    for kwargs, code in ((dict(width=64, height=64, upscale=0.5, precision=1), 3), (dict(width=8400, height=64, upscale=0.5), 2),
                         (dict(width=64, height=10240, upscale=0.5), 2),       # a column of 10240 points does not fit the LDS
                         (dict(width=64, height=64, upscale=1.5), 1), (dict(width=66, height=64, upscale=0.5), 1)):
        with pytest.raises(v.FftupError) as e:
            v.Upscaler(flags=v.FLAG_DOWNSCALE, **kwargs)
        assert e.value.code == code, kwargs
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(64, 64, 0.5)
    assert e.value.code == 1
