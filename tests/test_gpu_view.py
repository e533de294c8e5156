"""GPU: view plans (fftup_plan_create_view, Upscaler.view) -- the frame's trigonometric interpolant at origin + m span / M per axis,
computed as chirp-z transforms -- against the fp64 dense-matrix statement of the rule, tests/view_oracle.py, followed by
oraclelib.sharpen with the effective factor u_e = (float)sqrt(uW uH / (span_x span_y)) (quirks B4, B5).

Bars: those of tests/paritylib.py, the bars of the Bluestein and odd-size plans -- the construction is the same (a cyclic
convolution through two Stockham transforms of a smooth length, tables from the host).  The amplitude-preserving image is
sc * R, sc = uW uH / (span_x span_y)."""
import subprocess

import numpy as np
import pytest

import exactsize_oracle as E
import family_sweep_cases as F
import paritylib as P
import view_oracle as V
from paritylib import CLI

pytestmark = pytest.mark.gpu

# full-frame lattices: fold and split, an odd output row, kept Nyquist bins, a tail row, Bluestein forward transforms
FULL = [(50, 32, 32, 50, ""), (40, 30, 25, 48, ""), (64, 48, 64, 72, ""), (45, 21, 64, 21, ""), (46, 22, 70, 30, "any")]
# interior and wrapped views: a zoom inside the frame; a view wider than the frame that starts left of it; a band-limited view wider
# than the frame (steps 2.43 and 2); Bluestein forward transforms under a 3x zoom
VIEWS = [(48, 40, 40, 36, (10.3, 7.75), (17.9, 12.2), ""), (45, 21, 64, 30, (-3.25, 2.5), (61.5, 33.3), ""),
         (50, 32, 32, 20, (5.5, 0.0), (77.7, 40.0), ""), (46, 22, 70, 30, (0.4, 0.6), (23.0, 11.0), "any")]


def _flags(v, extra):
    return v.FLAG_ANY_SIZE if "any" in extra else 0


def _run(W, H, uW, uH, origin, span, precision, flags, rgb=None, planes=None):
    import vkresample_amd as v
    with v.Upscaler.view(W, H, uW, uH, origin, span, precision, P.SHARPEN, 0, flags) as up:
        pre, out = P.run_uploaded(up, rgb, planes)
        names, desc = up.kernel_names, up.description
        assert (up.out_width, up.out_height) == (uW, uH)
        assert not up.tuned and not up.u8_store and up.num_kernels == 4
    return pre, out, names, desc


def _check(W, H, uW, uH, origin, span, precision, extra, uint8, seed, tag, y=None, dense=True, pooled=None):
    """as tests/test_gpu_exactsize.py::_check; `y`: the amplitude-preserving image by another oracle (a function of the planes),
    compared with the dense statement as well -- or, with dense=False (lengths of thousands), in its place; `pooled`: a list that
    takes the -p 2 counts (differing, all) of R and of the output in place of the two fraction bars"""
    import vkresample_amd as v
    rgb, planes, x = P.inputs(W, H, precision, uint8, seed)
    pre, out, names, desc = _run(W, H, uW, uH, origin, span, precision, _flags(v, extra) | (v.FLAG_FUSE_U8_LOAD if uint8 else 0), rgb, planes)
    assert names[0] in ("row_r2c_odd", "row_r2c_odd_bz") and names[1] in ("col_view", "col_view_bz") and names[2:] == ["row_view_c2r", "sharpen"], names
    # (a Bluestein forward transform per axis whose input length is not smooth: FLAG_ANY_SIZE allows it, the lengths decide)
    assert ("_bz" in names[0]) == (not F.smooth(W)) and ("_bz" in names[1]) == (not F.smooth(H)), names
    assert "any" in extra or (F.smooth(W) and F.smooth(H))
    assert "rows %d->%d" % (W, uW) in desc and "columns %d->%d" % (H, uH) in desc and "origin" in desc and "span" in desc, desc
    sc = uW * uH / (span[0] * span[1])
    yv = V.view_planes(x, uW, uH, origin, span) if dense else y(x)
    u_e = V.effective_factor(uW, uH, span)
    assert pre.shape == yv.shape == (3, uH, uW)
    if y is not None and dense:
        assert np.abs(y(x) - yv).max() <= 1e-12                         # (the two oracles agree on this lattice)
    P.assert_parity(tag, precision, pre, out, yv, sc, u_e, pooled=pooled)
    return pre, x


@pytest.mark.parametrize("align", [E.ALIGN_CORNER, E.ALIGN_CENTRE])
@pytest.mark.parametrize("W,H,uW,uH,extra", FULL)
def test_full_frame_lattice_against_both_oracles(W, H, uW, uH, extra, align):
    """origin = the alignment's shift, span = the frame: the exact-size plans' map -- fold, split, kept Nyquist bin and the tail row"""
    _check(W, H, uW, uH, (E.delta(W, uW, align), E.delta(H, uH, align)), (float(W), float(H)), 0, extra, False, W + H + uW,
           "view full p0 %dx%d->%dx%d a%d %s" % (W, H, uW, uH, align, extra), y=lambda x: E.resample_planes(x, uW, uH, align))


# the full frame of 16x256 at 32x512: a thin frame whose column pass (convolution length 768, tiles of 8) needs 104 464 bytes of
# dynamic LDS -- above the 64 KB a kernel gets without its attribute
THIN = [(16, 256, 32, 512, (0.0, 0.0), (16.0, 256.0), "")]


@pytest.mark.parametrize("uint8", [False, True])
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("W,H,uW,uH,origin,span,extra", VIEWS + THIN)
def test_view_parity(W, H, uW, uH, origin, span, extra, precision, uint8):
    _check(W, H, uW, uH, origin, span, precision, extra, uint8, W + H + uW + precision,
           "view p%d %dx%d->%dx%d o%s s%s %s u8%d" % (precision, W, H, uW, uH, origin, span, extra, uint8))


@pytest.mark.parametrize("W,H,uW,uH,origin,span,extra", VIEWS)
def test_cosine_comes_back_at_the_view_positions(W, H, uW, uH, origin, span, extra):
    """what the oracle alone cannot hide: rows 0.5 + a cos(2 pi k x / W + 0.4) come back as the same cosine at x = origin + m span / uW,
    for k = 1 and the largest k the view copies whole (k <= kmax, below W/2)"""
    import vkresample_amd as v
    a, sc = 0.3, uW * uH / (span[0] * span[1])
    pos = V.positions(uW, origin[0], span[0])
    kk = V.kmax(W, uW, span[0])
    for k in (1, kk if 2 * kk < W else kk - 1):
        row = 0.5 + a * np.cos(2 * np.pi * k * np.arange(W) / W + 0.4)
        x = np.ascontiguousarray(np.broadcast_to(row, (3, H, W)).astype(np.float32))
        pre, _, _, _ = _run(W, H, uW, uH, origin, span, 0, _flags(v, extra), planes=x)
        want = np.broadcast_to(0.5 + a * np.cos(2 * np.pi * k * pos / W + 0.4), (3, uH, uW))
        # (the rows are cosines of the fp32 input, not of `row`: the interpolant of the rounding differences is within 2^-24 * a few)
        P.measured("view cosine %d->%d k=%d" % (W, uW, k), max_err=np.abs(sc * pre - want).max(), l2=P.rel_l2(sc * pre, want))
        assert P.rel_l2(sc * pre, want) <= P.FP32_PRE_L2
        assert np.abs(sc * pre - want).max() <= P.FP32_PRE_MAX


@pytest.mark.parametrize("W,H,uW,uH,origin,span,extra", VIEWS[:2])
def test_rolling_the_input_is_moving_the_origin(W, H, uW, uH, origin, span, extra):
    import vkresample_amd as v
    _, planes, _ = P.inputs(W, H, 0, False, 21)
    sc = uW * uH / (span[0] * span[1])
    a, _, _, _ = _run(W, H, uW, uH, (origin[0] + 3, origin[1] + 3), span, 0, _flags(v, extra), planes=planes)
    b, _, _, _ = _run(W, H, uW, uH, origin, span, 0, _flags(v, extra), planes=np.ascontiguousarray(np.roll(planes, (-3, -3), axis=(1, 2))))
    P.measured("view roll %dx%d->%dx%d" % (W, H, uW, uH), max_err=sc * np.abs(a - b).max(), l2=P.rel_l2(a, b))
    assert P.rel_l2(a, b) <= P.FP32_PRE_L2 and sc * np.abs(a - b).max() <= P.FP32_PRE_MAX


def test_largest_row_convolution():
    """4096x8 -> 4096x8, a half-pixel shift: the row convolution length is exactly 8192 (the oracle through FFTs: the dense matrix
    of this length takes a minute; tests/test_view_oracle.py keeps the two together)"""
    import vkresample_amd as v
    _check(4096, 8, 4096, 8, (0.5, 0.0), (4096.0, 8.0), 0, "", False, 5, "view p0 4096x8 half-pixel shift L=8192",
           y=lambda x: V.shift_planes(x, (0.5, 0.0)), dense=False)
    with v.Upscaler.view(4096, 8, 4096, 8, (0.5, 0.0), (4096.0, 8.0)) as up:
        assert "L=8192" in up.description


def test_set_view_gives_the_bytes_of_a_fresh_plan():
    import vkresample_amd as v
    W, H, uW, uH = 48, 40, 40, 36
    rgb = P.frame(W, H, seed=9)
    # a pan at the same span (only one table changes), a zoom out past the frame (fewer spectrum columns), back in (more)
    seq = [((10.3, 7.75), (17.9, 12.2)), ((11.05, 7.5), (17.9, 12.2)), ((-2.0, 1.0), (96.0, 50.0)), ((3.0, 4.0), (8.0, 6.0))]
    fresh = []
    for precision in (0, 2):
        for origin, span in seq:
            with v.Upscaler.view(W, H, uW, uH, origin, span, precision) as up:
                up.upload_rgb8(rgb)
                up.execute(1)
                fresh.append((up.download_planar().tobytes(), up.download_rgb8().tobytes(), up.description, up.kernel_min_bytes))
    k = 0
    for precision in (0, 2):
        with v.Upscaler.view(W, H, uW, uH, (0.0, 0.0), (float(W), float(H)), precision) as up:
            up.upload_rgb8(rgb)
            for origin, span in seq:
                up.set_view(origin, span)
                up.execute(1)
                assert up.download_planar().tobytes() == fresh[k][0], (precision, origin, span)
                assert up.download_rgb8().tobytes() == fresh[k][1]
                assert (up.description, up.kernel_min_bytes) == fresh[k][2:]
                k += 1
            # an invalid view is refused and the plan keeps its view
            with pytest.raises(v.FftupError) as e:
                up.set_view((0.0, 0.0), (float("nan"), 6.0))
            assert e.value.code == 1 and "finite" in str(e.value)
            with pytest.raises(v.FftupError) as e:
                up.set_view((0.0, 0.0), (8.0, 400.0))
            assert e.value.code == 1 and "span_y" in str(e.value)
            up.execute(1)
            assert up.download_planar().tobytes() == fresh[k - 1][0]
    for make in (lambda: v.Upscaler(64, 48, 2.0), lambda: v.Upscaler.to_size(50, 32, 32, 50)):
        with make() as up:
            with pytest.raises(v.FftupError) as e:
                up.set_view((0.0, 0.0), (32.0, 32.0))
            assert e.value.code == 1 and "not a view plan" in str(e.value)


@pytest.mark.parametrize("precision", [0, 2])
def test_execute_device_ring_and_download_rgb8(precision):
    """one view through fftup_execute_device (both formats), the ring and the host-streamed queue: the bytes of upload -> execute -> download"""
    import vkresample_amd as v
    from devimage import PLANAR, RGB8, device_run
    W, H, uW, uH, origin, span = 45, 21, 64, 30, (-3.25, 2.5), (61.5, 33.3)
    frames = [np.ascontiguousarray(P.frame(W, H, seed=40 + k)) for k in range(3)]
    with v.Upscaler.view(W, H, uW, uH, origin, span, precision, ring=3) as up:
        want8, wantp = [], []
        for f in frames:
            up.upload_rgb8(f)
            up.execute(1)
            want8.append(up.download_rgb8())
            wantp.append(up.download_planar().tobytes())
        got, clean = device_run(up, RGB8, frames[1], RGB8)
        assert clean and got.tobytes() == want8[1].tobytes()
        got, clean = device_run(up, RGB8, frames[2], PLANAR, out_padded=True)
        assert clean and got.tobytes() == wantp[2]
        for s, f in enumerate(frames):
            up.upload_rgb8(f, s)
        up.execute_ring(3)
        for s in range(3):
            assert up.download_planar(s).tobytes() == wantp[s], s
        out = np.empty((uH, uW, 3), np.uint8)
        up.wait(up.submit_rgb8(frames[2], out))
        assert np.array_equal(out, want8[2])
        ms = up.profile_kernels(2)
        assert all(t > 0 for t in list(ms)[:4])


def test_view_cli(tmp_path):
    """-size 40x36 -view 10.3,7.75,17.9,12.2 on a 48x40 PNG gives the API's pixels; -view without -size, with -centres or malformed
    exits 1 with a message and writes nothing"""
    import vkresample_amd as v
    rgb = P.frame(48, 40, seed=78)
    with v.Upscaler.view(48, 40, 40, 36, (10.3, 7.75), (17.9, 12.2)) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        want = up.download_rgb8()
    P.png_write(tmp_path / "in.png", rgb)

    def cli(*args):
        return subprocess.run([CLI] + list(args), capture_output=True, text=True, cwd=tmp_path, timeout=120)

    r = cli("-i", "in.png", "-o", "out.png", "-size", "40x36", "-view", "10.3,7.75,17.9,12.2", "-n", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "48x40 to 40x36" in r.stdout and "view" in r.stdout
    assert np.array_equal(P.png_read(tmp_path / "out.png"), want)
    for bad in (["-view", "10.3,7.75,17.9,12.2", "-u", "2"], ["-size", "40x36", "-centres", "-view", "10.3,7.75,17.9,12.2"],
                ["-size", "40x36", "-view", "10.3,7.75,17.9"], ["-size", "40x36", "-view", "0,0,9000,12"]):
        r = cli("-i", "in.png", "-o", "bad.png", *bad)
        assert r.returncode != 0 and not (tmp_path / "bad.png").exists(), bad


def test_existing_plans_give_the_same_bytes_beside_a_view_plan():
    """a plan of fftup_plan_create and one of fftup_plan_create_size before, while and after a view plan exists in the process"""
    import vkresample_amd as v
    rgb, rgb2 = P.frame(240, 126, seed=7), P.frame(50, 32, seed=8)

    def both():
        got = []
        for make, f in ((lambda: v.Upscaler(240, 126, 2.0, 0, 0.2, 0, v.FLAG_GENERIC_KERNELS), rgb), (lambda: v.Upscaler(240, 126, 2.0, 2), rgb),
                        (lambda: v.Upscaler.to_size(50, 32, 32, 50, align=E.ALIGN_CENTRE), rgb2)):
            with make() as up:
                up.upload_rgb8(f)
                up.execute(1)
                got.append((up.download_planar().tobytes(), up.kernel_names, up.description))
        return got

    before = both()
    with v.Upscaler.view(50, 32, 32, 20, (5.5, 0.0), (77.7, 40.0)) as vp:
        vp.upload_rgb8(rgb2)
        vp.execute(1)
        during = both()
        vp.set_view((1.0, 2.0), (50.0, 32.0))
        vp.execute(1)
    assert before == during == both()
