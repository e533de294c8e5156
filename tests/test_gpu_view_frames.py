"""GPU: fftup_execute_device_views -- a view per frame on a view plan, the chirp tables of each frame built on the device by
k_view_tables ahead of the frame's kernels -- against the oracles of the view plans (tests/view_oracle.py, tests/mirror_oracle.py)
at the bars of tests/paritylib.py, unchanged (only the call's last frame has a pre-sharpen image: the others are held to the output
bars alone).  And against a fresh plan created with the frame's view (host tables): the two table sets differ by single fp32
rounding steps in a few entries, so the fp32 planes agree to relative L2 2e-7 -- about one rounding step; for -p 2 the fraction of
differing values is reported."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import paritylib as P
import view_oracle as V
from devimage import ESZ, FILL, PLANAR, RGB8, Image
from paritylib import CLI
from test_gpu_mirror import _oracle_y as _mirror_y
from test_host_mirror import _longdouble_tables as _mirror_tables

pytestmark = pytest.mark.gpu

W, H, UW, UH = 48, 40, 40, 36
# frame i runs on lane i % 3 (FFTUP_STREAMS, default 3): the four views of test_set_view_gives_the_bytes_of_a_fresh_plan (a pan, a
# zoom out past the frame, a zoom in); frame 4 has frame 1's span at another origin, three frames later on the same lane (only
# `pre` is rebuilt); frame 5 zooms in right behind frame 2's zoom out on lane 2 (more spectrum columns than the lane's last frame
# wrote); the whole frame
MOVING = [((10.3, 7.75), (17.9, 12.2)), ((11.05, 7.5), (17.9, 12.2)), ((-2.0, 1.0), (96.0, 50.0)), ((3.0, 4.0), (8.0, 6.0)),
          ((12.5, 6.25), (17.9, 12.2)), ((20.0, 10.0), (9.5, 7.0)), ((0.0, 0.0), (48.0, 40.0))]


def _views_run(up, frames, fmt_in, views, fmt_out=PLANAR):
    """frames[i] (rgb or planes, by fmt_in) through ONE execute_device_views call -> (per frame the output in dense order, the
    pre-sharpen image of the call's last frame); the bytes around every image must stay untouched"""
    esz = ESZ[up.precision]
    src = [Image(fmt_in, up.width, up.height, esz, False, frame=f) for f in frames]
    dst = [Image(fmt_out, up.out_width, up.out_height, esz) for _ in frames]
    try:
        up.execute_device_views([s.image for s in src], [d.image for d in dst], views)
        outs = []
        for d in dst:
            got, clean = d.read()
            assert clean
            outs.append(got.view(np.uint8) if fmt_out == RGB8 else got.view({0: np.float32, 2: np.float16}[up.precision]).reshape(3, up.out_height, up.out_width))
        return outs, up.download_presharpen().astype(np.float64)
    finally:
        for im in src + dst:
            im.close()


def _fresh(shape, view, precision, flags, frame, fmt_in):
    """the planes of a plan created with `view` (host tables)"""
    import vkresample_amd as v
    with v.Upscaler.view(*shape, view[0], view[1], precision, 0.2, 0, flags | (v.FLAG_FUSE_U8_LOAD if fmt_in == RGB8 else 0)) as up:
        if fmt_in == RGB8:
            up.upload_rgb8(frame)
        else:
            up.upload_planar(frame)
        up.execute(1)
        return up.download_planar()


def _against_fresh(tag, precision, out, fresh):
    if precision == 0:
        P.measured(tag, fresh_l2=P.rel_l2(out.astype(np.float64), fresh.astype(np.float64)), fresh_diff_frac=(out != fresh).mean())
        assert P.rel_l2(out.astype(np.float64), fresh.astype(np.float64)) <= 2e-7
    else:
        P.measured(tag, fresh_diff_frac=(out != fresh).mean())


def _moving(precision, fmt_in):
    import vkresample_amd as v
    uploads, xs = [], []
    for k in range(len(MOVING)):
        rgb, planes, x = P.inputs(W, H, precision, fmt_in == RGB8, 60 + k)
        uploads.append(rgb if fmt_in == RGB8 else planes)
        xs.append(x)
    ys = [V.view_planes(x, UW, UH, o, s) for x, (o, s) in zip(xs, MOVING)]
    # (8-bit input: read by the row kernel itself, as in tests/test_gpu_view.py)
    with v.Upscaler.view(W, H, UW, UH, (0.0, 0.0), (float(W), float(H)), precision, 0.2, 0, v.FLAG_FUSE_U8_LOAD if fmt_in == RGB8 else 0) as up:
        # the call's first n frames, n = 1 .. 7: the pre-sharpen tap is the last frame's, so every frame is the last one once
        for n in range(1, len(MOVING) + 1):
            outs, pre = _views_run(up, uploads[:n], fmt_in, MOVING[:n])
            for k in (range(n) if n == len(MOVING) else [n - 1]):
                (o, s) = MOVING[k]
                P.assert_parity("views p%d in%d frame %d of %d" % (precision, fmt_in, k, n), precision, pre if k == n - 1 else None, outs[k], ys[k],
                                UW * UH / (s[0] * s[1]), V.effective_factor(UW, UH, s))
    for k, view in enumerate(MOVING):
        _against_fresh("views p%d in%d frame %d" % (precision, fmt_in, k), precision, outs[k], _fresh((W, H, UW, UH), view, precision, 0, uploads[k], fmt_in))


@pytest.mark.parametrize("fmt_in", [RGB8, PLANAR], ids=["rgb8", "planar"])
@pytest.mark.parametrize("precision", [0, 2])
def test_a_moving_view(precision, fmt_in, monkeypatch):
    monkeypatch.setenv("FFTUP_STREAMS", "3")
    _moving(precision, fmt_in)


@pytest.mark.parametrize("precision", [0, 2])
def test_a_moving_view_on_one_lane(precision, monkeypatch):
    """every frame rewrites the same table set; frames 0 -> 1 are a pan on it"""
    monkeypatch.setenv("FFTUP_STREAMS", "1")
    _moving(precision, PLANAR)


@pytest.mark.parametrize("precision", [0, 2])
def test_mirror_views(precision):
    """46x22 -> 70x30 (Bluestein forward transforms), reflection instead of the wrap: an origin left of the frame, a span wider than
    the frame, the DCT lattice, a pan of it, a zoom"""
    import vkresample_amd as v
    w, h, uw, uh = 46, 22, 70, 30
    views = [((-3.25, 0.6), (23.0, 11.0)), ((0.37, -0.5), (61.5, 33.3)), (((w / uw - 1) / 2, (h / uh - 1) / 2), (float(w), float(h))),
             ((1.5, 0.25), (float(w), float(h))), ((10.3, 7.75), (17.9, 12.2))]
    flags = v.FLAG_MIRROR | v.FLAG_ANY_SIZE
    uploads, xs = [], []
    for k in range(len(views)):
        _, planes, x = P.inputs(w, h, precision, False, 80 + k)
        uploads.append(planes)
        xs.append(x)
    with v.Upscaler.view(w, h, uw, uh, (0.0, 0.0), (float(w), float(h)), precision, 0.2, 0, flags) as up:
        assert "mirror" in up.description
        for n in (3, len(views)):
            outs, pre = _views_run(up, uploads[:n], PLANAR, views[:n])
            for k in (range(n) if n == len(views) else [n - 1]):
                (o, s) = views[k]
                P.assert_parity("mirror views p%d frame %d of %d" % (precision, k, n), precision, pre if k == n - 1 else None, outs[k],
                                _mirror_y(xs[k], uw, uh, o, s), uw * uh / (s[0] * s[1]), V.effective_factor(uw, uh, s))
    for k, view in enumerate(views):
        _against_fresh("mirror views p%d frame %d" % (precision, k), precision, outs[k], _fresh((w, h, uw, uh), view, precision, flags, uploads[k], PLANAR))


def test_longest_convolution():
    """4096x8 -> 4096x8: L = 8192, the device's fp64 transform at its longest.  Frame 0 is the half-pixel shift of
    tests/test_gpu_view.py::test_largest_row_convolution (the oracle through FFTs), frame 1 a 2x zoom against a fresh plan"""
    import vkresample_amd as v
    w, h = 4096, 8
    views = [((0.5, 0.0), (4096.0, 8.0)), ((1000.25, 0.0), (2048.0, 8.0))]
    ins = []
    for k in range(2):
        _, planes, x = P.inputs(w, h, 0, False, 5 + k)
        ins.append((planes, x))
    with v.Upscaler.view(w, h, w, h, (0.0, 0.0), (float(w), float(h))) as up:
        assert "L=8192" in up.description
        outs, pre = _views_run(up, [ins[0][0]], PLANAR, views[:1])
        P.assert_parity("views 4096x8 half-pixel shift L=8192", 0, pre, outs[0], V.shift_planes(ins[0][1], (0.5, 0.0)), 1.0, V.effective_factor(w, h, views[0][1]))
        first = outs[0].tobytes()
        outs, _ = _views_run(up, [i[0] for i in ins], PLANAR, views)
        assert outs[0].tobytes() == first
    _against_fresh("views 4096x8 span 2048", 0, outs[1], _fresh((w, h, w, h), views[1], 0, 0, ins[1][0], PLANAR))


def _table_bars(tag, got, want):
    kmax, pre, post, bhat = got
    k, opre, opost, oc = want
    assert kmax == k
    K, M, L = 2 * k + 1, len(post), len(bhat)
    cw = np.zeros(L, np.complex128)
    cw[np.arange(-(K - 1), M) % L] = oc.astype(np.complex128)
    for name, a, b in (("pre", pre, opre.astype(np.complex128)), ("post", post, opost.astype(np.complex128)), ("bhat", bhat, np.fft.ifft(cw))):
        assert a.shape == b.shape
        a = a.astype(np.complex128)
        worst = max(np.abs(a.real - b.real).max(), np.abs(a.imag - b.imag).max())
        top = max(np.abs(b.real).max(), np.abs(b.imag).max())
        P.measured("%s %s" % (tag, name), max_diff=worst, max_table=top, steps=worst / top * 2.0 ** 23)
        assert worst <= 2.0 ** -23 * top


def test_tables_against_longdouble_numpy(monkeypatch):
    """what the lanes hold after a call, both axes: every entry within one fp32 rounding step (2^-23 max |table|) of a longdouble
    evaluation of the header's formulas; kmax by the header's rule.  A periodic plan (frames 3 and 4 are lane 0's and lane 1's
    last: a zoom, and a pan that rebuilt only `pre` beside chirp tables two frames old) and a mirror plan on one lane"""
    import vkresample_amd as v
    monkeypatch.setenv("FFTUP_STREAMS", "3")
    frames = [P.inputs(W, H, 0, False, 30 + k)[1] for k in range(5)]
    with v.Upscaler.view(W, H, UW, UH, (0.0, 0.0), (float(W), float(H))) as up:
        with pytest.raises(v.FftupError) as e:
            up.download_view_tables(0, 0)
        assert e.value.code == 1 and "no tables" in str(e.value)
        _views_run(up, frames, PLANAR, MOVING[:5])
        for lane, (o, s) in ((0, MOVING[3]), (1, MOVING[4]), (2, MOVING[2])):
            _table_bars("tables lane %d x" % lane, up.download_view_tables(lane, 0), V.chirp_tables(W, UW, o[0], s[0]))
            _table_bars("tables lane %d y" % lane, up.download_view_tables(lane, 1), V.chirp_tables(H, UH, o[1], s[1]))
        for lane, axis in ((3, 0), (0, 2)):
            with pytest.raises(v.FftupError) as e:
                up.download_view_tables(lane, axis)
            assert e.value.code == 1
    w, h, uw, uh = 46, 22, 70, 30
    view = ((-3.25, 0.6), (61.5, 11.0))
    with v.Upscaler.view(w, h, uw, uh, (0.0, 0.0), (float(w), float(h)), 0, 0.2, 0, v.FLAG_MIRROR | v.FLAG_ANY_SIZE) as up:
        _views_run(up, [P.inputs(w, h, 0, False, 36)[1]], PLANAR, [view])
        _table_bars("tables mirror x", up.download_view_tables(0, 0), _mirror_tables(w, uw, view[0][0], view[1][0]))
        _table_bars("tables mirror y", up.download_view_tables(0, 1), _mirror_tables(h, uh, view[0][1], view[1][1]))
    with v.Upscaler(64, 48, 2.0) as up:
        with pytest.raises(v.FftupError) as e:
            up.download_view_tables(0, 0)
        assert e.value.code == 1 and "not a view plan" in str(e.value)


def test_the_plan_keeps_its_view():
    import vkresample_amd as v
    rgb = P.frame(W, H, seed=9)
    own = ((10.3, 7.75), (17.9, 12.2))
    frames = [P.inputs(W, H, 0, False, 50 + k)[1] for k in range(4)]
    with v.Upscaler.view(W, H, UW, UH, own[0], own[1]) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        before = (up.download_planar().tobytes(), up.description, up.kernel_min_bytes)
        outs, pre = _views_run(up, frames, PLANAR, MOVING[2:6])
        # the tap is the call's last frame: its sharpened image is that frame's output
        s = MOVING[5][1]
        P.assert_parity("tap after views", 0, pre, outs[3], V.view_planes(frames[3].astype(np.float64), UW, UH, MOVING[5][0], s), UW * UH / (s[0] * s[1]),
                        V.effective_factor(UW, UH, s))
        buf = C.create_string_buffer(512)
        assert up._lib.fftup_plan_describe(up._h, buf, 512) == 0 and buf.value.decode() == before[1]
        up.execute(1)
        assert up.download_planar().tobytes() == before[0]
        up.set_view(own[0], own[1])
        up.execute(1)
        assert (up.download_planar().tobytes(), up.description, up.kernel_min_bytes) == before
        # ... and set_view still re-aims the plan as it did
        up.set_view(*MOVING[3])
        up.execute(1)
        moved = up.download_planar().tobytes()
    with v.Upscaler.view(W, H, UW, UH, *MOVING[3]) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        assert up.download_planar().tobytes() == moved


def test_refusals_leave_the_outputs_untouched():
    import vkresample_amd as v
    nan = float("nan")

    def refused(up, views, *words):
        frames = [P.inputs(up.width, up.height, 0, False, 70 + k)[1] for k in range(len(views))]
        src = [Image(PLANAR, up.width, up.height, 4, False, frame=f) for f in frames]
        dst = [Image(PLANAR, up.out_width, up.out_height, 4) for _ in frames]
        try:
            with pytest.raises(v.FftupError) as e:
                up.execute_device_views([s.image for s in src], [d.image for d in dst], views)
            assert e.value.code == 1, str(e.value)
            for w in words:
                assert w in str(e.value), str(e.value)
            for d in dst:
                assert (d.buf.download() == FILL).all()
        finally:
            for im in src + dst:
                im.close()

    with v.Upscaler(64, 48, 2.0) as up:
        refused(up, [((0.0, 0.0), (64.0, 48.0))], "not a view plan")
    with v.Upscaler.view(W, H, UW, UH, *MOVING[0]) as up:
        refused(up, [MOVING[0], MOVING[1], ((nan, 0.0), (17.9, 12.2)), MOVING[3]], "finite", "views[2]")
        refused(up, [MOVING[0], ((0.0, 0.0), (9.0 * UW, 12.2))], "span_x", "views[1]")
        refused(up, [((0.0, 0.0), (17.9, 9.0 * UH))], "span_y", "views[0]")
        src = Image(PLANAR, W, H, 4, False, frame=P.inputs(W, H, 0, False, 70)[1])
        dst = Image(PLANAR, UW, UH, 4)
        try:
            a, b = (v._lib.DeviceImageDesc * 1)(src.image.desc()), (v._lib.DeviceImageDesc * 1)(dst.image.desc())
            assert up._lib.fftup_execute_device_views(up._h, a, b, None, 1, None) == 1 and b"views is null" in up._lib.fftup_last_error()
            assert (dst.buf.download() == FILL).all()
        finally:
            src.close()
            dst.close()


def test_view_clip_cli(tmp_path):
    """-viewto ... -frames 4: four files, each the bytes of execute_device_views fed the doubles of the printed `view k:` lines; the
    bad invocations exit non-zero and write nothing"""
    import vkresample_amd as v
    rgb = P.frame(W, H, seed=78)
    P.png_write(tmp_path / "in.png", rgb)

    def cli(*args):
        return subprocess.run([CLI] + list(args), capture_output=True, text=True, cwd=tmp_path, timeout=120)

    r = cli("-i", "in.png", "-o", "clip.png", "-size", "40x36", "-view", "10.3,7.75,17.9,12.2", "-viewto", "3,4,8,6", "-frames", "4")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^view (\d+): (\S+) (\S+) (\S+) (\S+)$", r.stdout, re.M)
    assert [int(t[0]) for t in lines] == [0, 1, 2, 3]
    views = [((float(t[1]), float(t[2])), (float(t[3]), float(t[4]))) for t in lines]
    assert views == v.views_between(((10.3, 7.75), (17.9, 12.2)), ((3.0, 4.0), (8.0, 6.0)), 4)
    assert sorted(p.name for p in tmp_path.glob("clip*")) == ["clip_%04d.png" % k for k in range(1, 5)]
    with v.Upscaler.view(W, H, UW, UH, *views[0]) as up:
        outs, _ = _views_run(up, [rgb] * 4, RGB8, views, RGB8)
    for k in range(4):
        assert np.array_equal(P.png_read(tmp_path / ("clip_%04d.png" % (k + 1))), outs[k].reshape(UH, UW, 3)), k
    for bad in (["-size", "40x36", "-viewto", "3,4,8,6", "-frames", "4"], ["-size", "40x36", "-view", "10.3,7.75,17.9,12.2", "-viewto", "3,4,8,6"],
                ["-size", "40x36", "-view", "10.3,7.75,17.9,12.2", "-viewto", "3,4,8", "-frames", "4"],
                ["-size", "40x36", "-view", "10.3,7.75,17.9,12.2", "-viewto", "3,4,8,6", "-frames", "1"]):
        r = cli("-i", "in.png", "-o", "bad.png", *bad)
        assert r.returncode != 0 and not list(tmp_path.glob("bad*")), bad
