"""GPU: view plans with FFTUP_FLAG_MIRROR (Upscaler.view(..., flags=FLAG_MIRROR)) -- the view of the frame's half-sample even
reflection -- against the fp64 cosine-form statement of the rule, tests/mirror_oracle.py, followed by oraclelib.sharpen with the view
plans' effective factor (quirks B4, B5), at the bars of tests/paritylib.py, unchanged.  The amplitude-preserving image is
sc * R, sc = uW uH / (span_x span_y).

Without the mode the library ignores the bit and returns the periodic view: every parity, cross-check, border and name test below
then fails."""
import functools
import subprocess

import numpy as np
import pytest

import mirror_oracle as Mo
import paritylib as P
import view_oracle as V
from paritylib import CLI, smooth

pytestmark = pytest.mark.gpu


def _centre(N, M):
    return Mo.centre_origin(N, M)


# (W, H, uW, uH, origin, span, extra): an interior zoom, even lengths; odd lengths, the origin outside the frame and span > N (the
# view shows the reflections); Bluestein forward transforms; steps above 1 on both axes with an odd uH (tail row; kmax_x = W/2);
# steps above 2 (kmax_x < W/2: the truncated column count, one tile of 8 and a partial one); a thin frame with long columns
# (TK > 1, a partial last tile, dynamic LDS above 64 KB)
ZOOM = (48, 40, 40, 36, (10.3, 7.75), (17.9, 12.2), "")
REFLECTED = (45, 21, 64, 30, (-3.25, 2.5), (61.5, 33.3), "")
BLUESTEIN = (46, 22, 70, 30, (0.37, -0.5), (46.0, 22.0), "any")
DOWN = (50, 32, 25, 15, (_centre(50, 25), _centre(32, 15)), (50.0, 32.0), "")
DOWN3 = (50, 32, 20, 11, (_centre(50, 20), _centre(32, 11)), (50.0, 32.0), "")
THIN = (16, 256, 32, 512, (0.0, 0.0), (16.0, 256.0), "")
SHAPES = [ZOOM, REFLECTED, BLUESTEIN, DOWN, DOWN3, THIN]


def _flags(v, extra):
    return v.FLAG_MIRROR | (v.FLAG_ANY_SIZE if "any" in extra else 0)


@functools.lru_cache(maxsize=None)
def _matrix(N, M, origin, span):
    """the oracle's matrix of one axis, computed once per (axis, view) and shared by the tests; read-only"""
    A = Mo.mirror_matrix(N, M, origin, span)
    A.setflags(write=False)
    return A


def _oracle_y(x, uW, uH, origin, span):
    _, H, W = x.shape
    return _matrix(H, uH, origin[1], span[1]) @ x @ _matrix(W, uW, origin[0], span[0]).T


def _run(W, H, uW, uH, origin, span, precision, flags, rgb=None, planes=None):
    import vkresample_amd as v
    with v.Upscaler.view(W, H, uW, uH, origin, span, precision, P.SHARPEN, 0, flags) as up:
        pre, out = P.run_uploaded(up, rgb, planes)
        names, desc = up.kernel_names, up.description
        assert (up.out_width, up.out_height) == (uW, uH)
        assert not up.tuned and not up.u8_store and up.num_kernels == 4
    return pre, out, names, desc


def _check(W, H, uW, uH, origin, span, precision, extra, uint8, seed, tag):
    import vkresample_amd as v
    rgb, planes, x = P.inputs(W, H, precision, uint8, seed)
    pre, out, names, desc = _run(W, H, uW, uH, origin, span, precision, _flags(v, extra) | (v.FLAG_FUSE_U8_LOAD if uint8 else 0), rgb, planes)
    assert names == ["row_r2c_mirror" + ("" if smooth(W) else "_bz"), "col_view_mirror" + ("" if smooth(H) else "_bz"), "row_view_c2r_mirror", "sharpen"], names
    assert "mirror" in desc and "rows %d->%d" % (W, uW) in desc and "columns %d->%d" % (H, uH) in desc, desc
    sc = uW * uH / (span[0] * span[1])
    yv = _oracle_y(x, uW, uH, origin, span)
    u_e = V.effective_factor(uW, uH, span)
    assert pre.shape == yv.shape == (3, uH, uW)
    P.assert_parity(tag, precision, pre, out, yv, sc, u_e)
    return pre, x


@pytest.mark.parametrize("uint8", [False, True])
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("W,H,uW,uH,origin,span,extra", SHAPES)
def test_mirror_parity(W, H, uW, uH, origin, span, extra, precision, uint8):
    _check(W, H, uW, uH, origin, span, precision, extra, uint8, W + H + uW + precision,
           "mirror p%d %dx%d->%dx%d o%s s%s %s u8%d" % (precision, W, H, uW, uH, origin, span, extra, uint8))


def test_largest_row_convolution():
    """2048x16 -> 4096x16, centre-aligned along x: the row convolution length is exactly 8192"""
    import vkresample_amd as v
    _check(2048, 16, 4096, 16, (_centre(2048, 4096), 0.0), (2048.0, 16.0), 0, "", False, 5, "mirror p0 2048x16->4096x16 L=8192")
    with v.Upscaler.view(2048, 16, 4096, 16, (_centre(2048, 4096), 0.0), (2048.0, 16.0), flags=v.FLAG_MIRROR) as up:
        assert "L=8192" in up.description


@pytest.mark.parametrize("W,H,uW,uH,origin,span,extra", [ZOOM, REFLECTED, BLUESTEIN])
def test_mirror_plan_against_the_periodic_plan_on_the_extended_frame(W, H, uW, uH, origin, span, extra):
    """no oracle: the existing periodic view plan, fed the explicit 2W x 2H even extension built on the host, computes the same
    numbers with the same view and output size.  The pre-sharpen images agree within the sum of the two plans' parity bounds"""
    import vkresample_amd as v
    _, planes, _ = P.inputs(W, H, 0, False, 31)
    ext = np.ascontiguousarray(Mo.extend(Mo.extend(planes, 2), 1))
    assert ext.shape == (3, 2 * H, 2 * W) and np.array_equal(ext[:, 2 * H - 1, 2 * W - 1], planes[:, 0, 0])
    a, _, names, _ = _run(W, H, uW, uH, origin, span, 0, _flags(v, extra), planes=planes)
    b, _, pnames, _ = _run(2 * W, 2 * H, uW, uH, origin, span, 0, _flags(v, extra) & ~v.FLAG_MIRROR, planes=ext)
    assert "_mirror" in names[0] and "_mirror" not in pnames[0]
    sc = uW * uH / (span[0] * span[1])
    P.measured("mirror vs periodic-on-extension %dx%d->%dx%d" % (W, H, uW, uH), l2=P.rel_l2(a, b), max_err=sc * np.abs(a - b).max())
    assert P.rel_l2(a, b) <= 2 * P.FP32_PRE_L2 and sc * np.abs(a - b).max() <= 2 * P.FP32_PRE_MAX


def test_centre_alignment_is_the_dct_mode():
    """40x24 at u = 2, origin = (N/M - 1)/2, span = the frame: the pre-sharpen image of a FFTUP_FLAG_DCT plan on the same frame"""
    import vkresample_amd as v
    W, H, uW, uH = 40, 24, 80, 48
    _, planes, x = P.inputs(W, H, 0, False, 12)
    a, _, _, _ = _run(W, H, uW, uH, (_centre(W, uW), _centre(H, uH)), (float(W), float(H)), 0, v.FLAG_MIRROR, planes=planes)
    with v.Upscaler(W, H, 2.0, 0, 0.2, 0, v.FLAG_DCT) as up:
        up.upload_planar(planes)
        up.execute(1)
        b = up.download_presharpen().astype(np.float64)
    sc = 4.0
    P.measured("mirror centre-aligned vs dct 40x24 u2", l2=P.rel_l2(a, b), max_err=sc * np.abs(a - b).max())
    assert P.rel_l2(a, b) <= P.FP32_PRE_L2 and sc * np.abs(a - b).max() <= P.FP32_PRE_MAX


def test_border_of_a_ramp():
    """a horizontal ramp 32x16 -> 64x32, centre-aligned: the periodic view rings at the jump between the last and the first column,
    the mirror view has no jump"""
    import vkresample_amd as v
    W, H, uW, uH = 32, 16, 64, 32
    planes = np.ascontiguousarray(np.broadcast_to(np.linspace(0, 1, W), (3, H, W)).astype(np.float32))
    origin, span, sc = (_centre(W, uW), _centre(H, uH)), (float(W), float(H)), 4.0
    mir, _, _, _ = _run(W, H, uW, uH, origin, span, 0, v.FLAG_MIRROR, planes=planes)
    per, _, _, _ = _run(W, H, uW, uH, origin, span, 0, 0, planes=planes)
    P.measured("ramp 32->64", mirror_min=(sc * mir).min(), mirror_max=(sc * mir).max(), periodic_min=(sc * per).min(), periodic_max=(sc * per).max())
    assert (sc * mir).min() >= -0.01 and (sc * mir).max() <= 1.01
    assert (sc * per).min() < -0.1 and (sc * per).max() > 1.1


def test_set_view_gives_the_bytes_of_a_fresh_plan():
    import vkresample_amd as v
    W, H, uW, uH = 48, 40, 40, 36
    rgb = P.frame(W, H, seed=9)
    # a pan at the same span (only one table changes), a zoom out past the frame (fewer spectrum columns), back in (more)
    seq = [((10.3, 7.75), (17.9, 12.2)), ((11.05, 7.5), (17.9, 12.2)), ((-2.0, 1.0), (150.0, 50.0)), ((3.0, 4.0), (8.0, 6.0))]
    fresh = []
    for precision in (0, 2):
        for origin, span in seq:
            with v.Upscaler.view(W, H, uW, uH, origin, span, precision, flags=v.FLAG_MIRROR) as up:
                up.upload_rgb8(rgb)
                up.execute(1)
                fresh.append((up.download_planar().tobytes(), up.download_rgb8().tobytes(), up.description, up.kernel_min_bytes))
    assert len({f[3][0] for f in fresh}) > 1                          # (the zoom out stores fewer columns)
    k = 0
    for precision in (0, 2):
        with v.Upscaler.view(W, H, uW, uH, (0.0, 0.0), (float(W), float(H)), precision, flags=v.FLAG_MIRROR) as up:
            up.upload_rgb8(rgb)
            for origin, span in seq:
                up.set_view(origin, span)
                up.execute(1)
                assert up.download_planar().tobytes() == fresh[k][0], (precision, origin, span)
                assert up.download_rgb8().tobytes() == fresh[k][1]
                assert (up.description, up.kernel_min_bytes) == fresh[k][2:]
                k += 1
            with pytest.raises(v.FftupError) as e:
                up.set_view((0.0, 0.0), (8.0, 400.0))
            assert e.value.code == 1 and "span_y" in str(e.value)
            up.execute(1)
            assert up.download_planar().tobytes() == fresh[k - 1][0]


@pytest.mark.parametrize("precision", [0, 2])
def test_execute_device_and_ring(precision):
    """one mirror view through fftup_execute_device (both formats), the ring and the host-streamed queue: the bytes of
    upload -> execute -> download"""
    import vkresample_amd as v
    from devimage import PLANAR, RGB8, device_run
    W, H, uW, uH, origin, span = REFLECTED[:6]
    frames = [np.ascontiguousarray(P.frame(W, H, seed=40 + k)) for k in range(3)]
    with v.Upscaler.view(W, H, uW, uH, origin, span, precision, flags=v.FLAG_MIRROR, ring=3) as up:
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


def test_mirror_cli(tmp_path):
    """-size 40x36 -view 10.3,7.75,17.9,12.2 -mirror on a 48x40 PNG gives the API's pixels; -mirror without a view exits 1 with a
    message and writes nothing"""
    import vkresample_amd as v
    rgb = P.frame(48, 40, seed=78)
    got = []
    for flags in (v.FLAG_MIRROR, 0):
        with v.Upscaler.view(48, 40, 40, 36, (10.3, 7.75), (17.9, 12.2), flags=flags) as up:
            up.upload_rgb8(rgb)
            up.execute(1)
            got.append(up.download_rgb8())
    want, periodic = got
    assert not np.array_equal(want, periodic)
    P.png_write(tmp_path / "in.png", rgb)

    def cli(*args):
        return subprocess.run([CLI] + list(args), capture_output=True, text=True, cwd=tmp_path, timeout=120)

    r = cli("-i", "in.png", "-o", "out.png", "-size", "40x36", "-view", "10.3,7.75,17.9,12.2", "-mirror", "-n", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(P.png_read(tmp_path / "out.png"), want)
    for bad in (["-u", "2", "-mirror"], ["-size", "40x36", "-mirror"], ["-size", "40x36", "-centres", "-mirror"]):
        r = cli("-i", "in.png", "-o", "bad.png", *bad)
        assert r.returncode == 1 and "-mirror needs" in r.stdout and not (tmp_path / "bad.png").exists(), bad
    assert "-mirror" in cli("-h").stdout


def test_existing_plans_give_the_same_bytes_beside_a_mirror_plan():
    """a periodic view plan and a -u 2 plan before, while and after a mirror plan exists in the process"""
    import vkresample_amd as v
    rgb, rgb2 = P.frame(240, 126, seed=7), P.frame(50, 32, seed=8)

    def both():
        got = []
        for make, f in ((lambda: v.Upscaler(240, 126, 2.0, 0, 0.2, 0), rgb), (lambda: v.Upscaler(240, 126, 2.0, 2), rgb),
                        (lambda: v.Upscaler.view(50, 32, 32, 20, (5.5, 0.0), (77.7, 40.0)), rgb2)):
            with make() as up:
                up.upload_rgb8(f)
                up.execute(1)
                got.append((up.download_planar().tobytes(), up.kernel_names, up.description))
        return got

    before = both()
    with v.Upscaler.view(50, 32, 32, 20, (5.5, 0.0), (77.7, 40.0), flags=v.FLAG_MIRROR) as mp:
        mp.upload_rgb8(rgb2)
        mp.execute(1)
        during = both()
        mp.set_view((1.0, 2.0), (50.0, 32.0))
        mp.execute(1)
        assert all("_mirror" in n for n in mp.kernel_names[:3]) and mp.kernel_names[3] == "sharpen"
    assert before == during == both()
    assert not any("_mirror" in n for g in before for n in g[1])
