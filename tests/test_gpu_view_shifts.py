"""GPU: fftup_execute_device_views_shifted -- a view per frame whose origin the frame's table kernel moves by a fftup_shift it reads
from device memory -- and fftup_shift_path, the kernel that turns measured shifts into the offsets of a smoothed camera path.

The shifted call is held to BYTES: frame i must be what fftup_execute_device_views gives for views[i] with the origin moved on the host,
in float64, by the float32 shift (a dx or dy that is not finite counts as 0) -- the same csrc/view_phase.hpp code on the same doubles.
One configuration is also held to the view oracle at the moved origins, at the bars of tests/paritylib.py unchanged, and its tables to
one fp32 rounding step.  The path kernel is held to tests/path_oracle.py at one fp32 rounding step, 2^-23 max(|oracle|, 1): its fp64 sums
of at most 4096 fp32 values carry errors below 1e-8, far under that step."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import align_oracle as AO
import paritylib as P
import path_oracle as PO
import view_oracle as V
from devimage import ESZ, FILL, GUARD, PLANAR, RGB8, Image
from paritylib import CLI
from test_gpu_view_frames import MOVING, _table_bars

pytestmark = pytest.mark.gpu

W, H, UW, UH = 48, 40, 40, 36
MW, MH, MUW, MUH = 46, 22, 70, 30
MIRROR_VIEWS = [((-3.25, 0.6), (23.0, 11.0)), ((0.37, -0.5), (61.5, 33.3)), (((MW / MUW - 1) / 2, (MH / MUH - 1) / 2), (float(MW), float(MH))),
                ((1.5, 0.25), (float(MW), float(MH))), ((10.3, 7.75), (17.9, 12.2))]
NAN, INF = float("nan"), float("inf")
# a whole pixel and more, a shift of a million periods' worth, not-a-number on one axis only, infinities, less than the origin's ulp
SHIFTS = [(0.0, 0.0), (1.3, -0.7), (-2.2, 1.6), (1e6 + 0.25, -3e5), (NAN, 2.5), (INF, -INF), (2.0 ** -30, -2.0 ** -30)]


def _shift_rows(pairs):
    """fftup_shift rows: dx, dy and a peak / peak_coarse the call must not read (NaN)"""
    rows = np.full((len(pairs), 4), np.nan, np.float32)
    rows[:, :2] = np.array(pairs, np.float32)
    return rows


def _moved(views, rows):
    """the views with their origins moved on the host: float64 + the float32 value widened, a value that is not finite as 0"""
    out = []
    for (o, s), row in zip(views, rows):
        d = [float(np.float64(x)) if math.isfinite(x) else 0.0 for x in row[:2]]
        out.append(((float(np.float64(o[0]) + np.float64(d[0])), float(np.float64(o[1]) + np.float64(d[1]))), s))
    return out


def _run(up, frames, fmt_in, views, rows=None, fmt_out=PLANAR, stream=None):
    """frames through ONE execute_device_views call, or with `rows` ((n, 4) float32, uploaded by hand) ONE execute_device_views_shifted
    call -> (per frame the output in dense order, the pre-sharpen image of the call's last frame); every guard byte must stay clean"""
    import vkresample_amd as v
    esz = ESZ[up.precision]
    src = [Image(fmt_in, up.width, up.height, esz, False, frame=f) for f in frames]
    dst = [Image(fmt_out, up.out_width, up.out_height, esz) for _ in frames]
    buf = None
    try:
        if rows is None:
            up.execute_device_views([s.image for s in src], [d.image for d in dst], views, stream)
        else:
            buf = v.DeviceBuffer(2 * GUARD + rows.nbytes)
            host = np.full(buf.nbytes, FILL, np.uint8)
            host[GUARD:GUARD + rows.nbytes] = rows.view(np.uint8).reshape(-1)
            buf.upload(host)
            up.execute_device_views_shifted([s.image for s in src], [d.image for d in dst], views, buf.ptr + GUARD, stream)
        outs = []
        for d in dst:
            got, clean = d.read(stream)
            assert clean
            outs.append(got.view(np.uint8) if fmt_out == RGB8 else got.view({0: np.float32, 2: np.float16}[up.precision]).reshape(3, up.out_height, up.out_width))
        if buf is not None:
            assert buf.download().tobytes() == host.tobytes()            # the shifts are only read
        return outs, up.download_presharpen().astype(np.float64)
    finally:
        for im in src + dst:
            im.close()
        if buf is not None:
            buf.close()


def _uploads(w, h, precision, fmt_in, n, seed):
    ups, xs = [], []
    for k in range(n):
        rgb, planes, x = P.inputs(w, h, precision, fmt_in == RGB8, seed + k)
        ups.append(rgb if fmt_in == RGB8 else planes)
        xs.append(x)
    return ups, xs


# ---------------------------------------------------------------- 1. the bytes of the host-shifted call
@pytest.mark.parametrize("streams", [3, 1])
@pytest.mark.parametrize("fmt_in", [RGB8, PLANAR], ids=["rgb8", "planar"])
@pytest.mark.parametrize("precision", [0, 2])
def test_bytes_of_the_host_shifted_call(precision, fmt_in, streams, monkeypatch):
    import vkresample_amd as v
    monkeypatch.setenv("FFTUP_STREAMS", str(streams))
    rows = _shift_rows(SHIFTS)
    uploads, _ = _uploads(W, H, precision, fmt_in, len(MOVING), 60)
    with v.Upscaler.view(W, H, UW, UH, (0.0, 0.0), (float(W), float(H)), precision, 0.2, 0, v.FLAG_FUSE_U8_LOAD if fmt_in == RGB8 else 0) as up:
        got, got_pre = _run(up, uploads, fmt_in, MOVING, rows)
        want, want_pre = _run(up, uploads, fmt_in, _moved(MOVING, rows))
    for k in range(len(MOVING)):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got_pre.tobytes() == want_pre.tobytes()


@pytest.mark.parametrize("streams", [3, 1])
@pytest.mark.parametrize("precision", [0, 2])
def test_bytes_of_the_host_shifted_call_mirror(precision, streams, monkeypatch):
    import vkresample_amd as v
    monkeypatch.setenv("FFTUP_STREAMS", str(streams))
    rows = _shift_rows(SHIFTS[1:6])
    uploads, _ = _uploads(MW, MH, precision, PLANAR, len(MIRROR_VIEWS), 80)
    with v.Upscaler.view(MW, MH, MUW, MUH, (0.0, 0.0), (float(MW), float(MH)), precision, 0.2, 0, v.FLAG_MIRROR | v.FLAG_ANY_SIZE) as up:
        assert "mirror" in up.description
        got, got_pre = _run(up, uploads, PLANAR, MIRROR_VIEWS, rows)
        want, want_pre = _run(up, uploads, PLANAR, _moved(MIRROR_VIEWS, rows))
    for k in range(len(MIRROR_VIEWS)):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got_pre.tobytes() == want_pre.tobytes()


def test_shifted_frames_against_the_view_oracle(monkeypatch):
    """-p 0, planes in, three lanes: every output and the last frame's pre-sharpen image against view_oracle.view_planes at the moved
    origins, paritylib's bars unchanged; the tables the lanes hold afterwards (frames 6, 4 and 5 on lanes 0, 1 and 2) within one fp32
    rounding step of the longdouble tables at the moved origins"""
    import vkresample_amd as v
    monkeypatch.setenv("FFTUP_STREAMS", "3")
    rows = _shift_rows(SHIFTS)
    moved = _moved(MOVING, rows)
    uploads, xs = _uploads(W, H, 0, PLANAR, len(MOVING), 60)
    with v.Upscaler.view(W, H, UW, UH, (0.0, 0.0), (float(W), float(H))) as up:
        outs, pre = _run(up, uploads, PLANAR, MOVING, rows)
        n = len(MOVING)
        for k, (o, s) in enumerate(moved):
            P.assert_parity("shifted views frame %d" % k, 0, pre if k == n - 1 else None, outs[k], V.view_planes(xs[k], UW, UH, o, s),
                            UW * UH / (s[0] * s[1]), V.effective_factor(UW, UH, s))
        for lane, k in ((0, 6), (1, 4), (2, 5)):
            (o, s) = moved[k]
            _table_bars("shifted tables lane %d x" % lane, up.download_view_tables(lane, 0), V.chirp_tables(W, UW, o[0], s[0]))
            _table_bars("shifted tables lane %d y" % lane, up.download_view_tables(lane, 1), V.chirp_tables(H, UH, o[1], s[1]))
    assert moved[4][0] == (12.5, 8.75) and moved[5] == MOVING[5] and moved[3][0] == (1000003.25, -299996.0)


# ---------------------------------------------------------------- 2. zero shifts, and the plan keeps its view
def test_zero_shifts_give_the_unshifted_bytes_and_the_plan_keeps_its_view():
    import vkresample_amd as v
    rgb = P.frame(W, H, seed=9)
    own = ((10.3, 7.75), (17.9, 12.2))
    frames = [P.inputs(W, H, 0, False, 50 + k)[1] for k in range(4)]
    with v.Upscaler.view(W, H, UW, UH, own[0], own[1]) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        before = (up.download_planar().tobytes(), up.description)
        plain, plain_pre = _run(up, frames, PLANAR, MOVING[2:6])
        zero, zero_pre = _run(up, frames, PLANAR, MOVING[2:6], np.zeros((4, 4), np.float32))
        for a, b in zip(plain, zero):
            assert a.tobytes() == b.tobytes()
        assert plain_pre.tobytes() == zero_pre.tobytes()
        up.execute(1)
        assert (up.download_planar().tobytes(), up.description) == before


# ---------------------------------------------------------------- 3. no host wait in the chain
SW, SH, SUW, SUH = 48, 40, 40, 36
STAB_SHIFTS = [(1.3, -0.7), (-2.2, 1.6), (2.75, 2.1), (-0.9, -2.6), (3.0, 0.4)]
STAB_VIEW = ((4.0, 2.0), (40.0, 36.0))


def test_the_chain_on_one_stream_without_a_host_wait():
    """estimates -> path (ABSOLUTE, sigma 0, in place) -> shifted views, all enqueued on one user stream with nothing between them but
    Python, ONE synchronisation at the end: the bytes of the synchronous chain Aligner.shifts -> stabilised_views -> execute_device_views"""
    import vkresample_amd as v
    frames = AO.clip(SW, SH, 1, [(0.0, 0.0)] + STAB_SHIFTS, seed=5)
    n = len(frames) - 1
    ims = [Image(RGB8, SW, SH, 1, frame=f) for f in frames]
    dst = [Image(PLANAR, SUW, SUH, 4) for _ in range(n)]
    try:
        with v.Aligner(SW, SH) as al, v.Upscaler.view(SW, SH, SUW, SUH, STAB_VIEW[0], STAB_VIEW[1], sharpen=0.0) as up, \
                v.Stream() as s, v.DeviceBuffer(16 * n) as buf:
            ins = [im.image for im in ims[1:]]
            al.shifts_device(ims[0].image, ins, buf.ptr, stream=s)
            v.shift_path(buf.ptr, buf.ptr, n, v.PATH_ABSOLUTE, 0.0, 0.0, stream=s)
            up.execute_device_views_shifted(ins, [d.image for d in dst], [STAB_VIEW] * n, buf.ptr, stream=s)
            chain = [d.read(stream=s) for d in dst]                      # (the first read-back waits for the stream: the one wait)
            est = al.shifts(ims[0].image, ins)
            assert buf.download().tobytes() == est.tobytes()
            want, _ = _run(up, [f for f in frames[1:]], RGB8, v.stabilised_views(STAB_VIEW, est))
        for k in range(n):
            assert chain[k][1] and chain[k][0].tobytes() == want[k].tobytes(), k
        assert np.abs(est[:, :2]).max() > 0.5
    finally:
        for im in ims + dst:
            im.close()


# ---------------------------------------------------------------- 4. the path kernel against the oracle
class _Guarded:
    """n fftup_shift in device memory between two guard bands of 0xA5"""

    def __init__(self, n, rows=None):
        import vkresample_amd as v
        self.n = n
        self.buf = v.DeviceBuffer(2 * GUARD + 16 * n)
        host = np.full(2 * GUARD + 16 * n, FILL, np.uint8)
        if rows is not None:
            host[GUARD:GUARD + 16 * n] = np.ascontiguousarray(rows, np.float32).view(np.uint8).reshape(-1)
        self.buf.upload(host)
        self.ptr = self.buf.ptr + GUARD

    def read(self):
        raw = self.buf.download()
        return raw[GUARD:GUARD + 16 * self.n].view(np.float32).reshape(self.n, 4).copy(), bool((raw[:GUARD] == FILL).all() and (raw[GUARD + 16 * self.n:] == FILL).all())

    def untouched(self):
        return bool((self.buf.download() == FILL).all())

    def close(self):
        self.buf.close()


@pytest.mark.parametrize("min_peak", PO.MIN_PEAKS)
@pytest.mark.parametrize("mode", PO.MODES, ids=["absolute", "consecutive"])
def test_the_path_kernel_against_the_oracle(mode, min_peak):
    """every (n, sigma) of path_oracle.GRID: dx, dy within 2^-23 max(|oracle|, 1) of the oracle; peak and peak_coarse copied bit for
    bit; the same call twice and the call in place give the same bytes; only n * 16 bytes change between the guards"""
    import vkresample_amd as v
    worst = 0.0
    for (n, sigma) in PO.GRID:
        sh, (p, s, want) = PO.grid_case(n, sigma, mode, min_peak)
        src, a, b = _Guarded(n, sh), _Guarded(n), _Guarded(n, sh)
        try:
            v.shift_path(src.ptr, a.ptr, n, mode, sigma, min_peak)
            first, first_ok = a.read()
            v.shift_path(src.ptr, a.ptr, n, mode, sigma, min_peak)
            again, again_ok = a.read()
            v.shift_path(b.ptr, b.ptr, n, mode, sigma, min_peak)
            inplace, inplace_ok = b.read()
            kept, kept_ok = src.read()
        finally:
            for g in (src, a, b):
                g.close()
        tag = (n, sigma, mode, min_peak)
        assert first_ok and again_ok and inplace_ok and kept_ok, tag
        assert kept.tobytes() == sh.tobytes(), tag
        assert first.tobytes() == again.tobytes() == inplace.tobytes(), tag
        assert first[:, 2:].tobytes() == sh[:, 2:].tobytes(), tag
        err = np.abs(first[:, :2].astype(np.float64) - want) / PO.out_bar(want)
        worst = max(worst, float(err.max()))
        assert np.isfinite(first[:, :2]).all() and (err <= 1.0).all(), (tag, float(err.max()))
    P.measured("shift_path mode %d min_peak %g" % (mode, min_peak), worst_over_bar=worst)


# ---------------------------------------------------------------- 5. refusals
def test_refusals_of_the_shifted_call_leave_the_outputs_untouched():
    import vkresample_amd as v
    host = np.zeros((8, 4), np.float32)

    def refused(up, views, shifts_ptr, *words):
        frames = [P.inputs(up.width, up.height, 0, False, 70 + k)[1] for k in range(len(views))]
        src = [Image(PLANAR, up.width, up.height, 4, False, frame=f) for f in frames]
        dst = [Image(PLANAR, up.out_width, up.out_height, 4) for _ in frames]
        try:
            with pytest.raises(v.FftupError) as e:
                up.execute_device_views_shifted([s.image for s in src], [d.image for d in dst], views, shifts_ptr)
            assert e.value.code == 1, str(e.value)
            for w in words:
                assert w in str(e.value), str(e.value)
            for d in dst:
                assert (d.buf.download() == FILL).all()
        finally:
            for im in src + dst:
                im.close()

    with v.DeviceBuffer(16 * 8) as good:
        good.upload(host)
        with v.Upscaler(64, 48, 2.0) as up:
            refused(up, [((0.0, 0.0), (64.0, 48.0))], good.ptr, "not a view plan")
        with v.Upscaler.view(W, H, UW, UH, *MOVING[0]) as up:
            # everything fftup_execute_device_views refuses ...
            refused(up, [MOVING[0], MOVING[1], ((NAN, 0.0), (17.9, 12.2)), MOVING[3]], good.ptr, "finite", "views[2]", "fftup_execute_device_views_shifted")
            refused(up, [MOVING[0], ((0.0, 0.0), (9.0 * UW, 12.2))], good.ptr, "span_x", "views[1]")
            # ... and the rules of shifts_device, in the words fftup_align_shifts has for its own
            refused(up, [MOVING[0]], None, "shifts_device is null")
            refused(up, [MOVING[0]], good.ptr + 2, "shifts_device is not a multiple of 4 bytes")
            refused(up, [MOVING[0]], host.ctypes.data, "shifts_device is not device memory")
            src = Image(PLANAR, W, H, 4, False, frame=P.inputs(W, H, 0, False, 70)[1])
            dst = Image(PLANAR, UW, UH, 4)
            try:
                a, b = (v._lib.DeviceImageDesc * 1)(src.image.desc()), (v._lib.DeviceImageDesc * 1)(dst.image.desc())
                assert up._lib.fftup_execute_device_views_shifted(up._h, a, b, None, good.ptr, 1, None) == 1 and b"views is null" in up._lib.fftup_last_error()
                c = (v._lib.View * 1)(v._lib.View(*MOVING[0][0], *MOVING[0][1]))
                assert up._lib.fftup_execute_device_views_shifted(up._h, a, b, c, good.ptr, 0, None) == 1 and b"n_frames must be > 0" in up._lib.fftup_last_error()
                assert (dst.buf.download() == FILL).all()
                # ... and the plan still serves the call
                up.execute_device_views_shifted(src.image, dst.image, [MOVING[0]], good.ptr)
                assert dst.read()[1] and not (dst.read()[0] == FILL).all()
            finally:
                src.close()
                dst.close()


def test_refusals_of_shift_path_leave_out_device_untouched():
    import vkresample_amd as v
    sh = PO.grid_shifts(8, 1)
    host = np.zeros((8, 4), np.float32)
    src, out = _Guarded(8, sh), _Guarded(8)
    try:
        bad = [
            (dict(n=0), "n_frames must be > 0"), (dict(n=4097), "above FFTUP_PATH_MAX_FRAMES"), (dict(mode=2), "mode must be"),
            (dict(sigma=-1.0), "sigma must be"), (dict(sigma=NAN), "sigma must be"), (dict(sigma=INF), "sigma must be"), (dict(sigma=257.0), "sigma must be"),
            (dict(min_peak=NAN), "min_peak must be"), (dict(min_peak=INF), "min_peak must be"),
            (dict(in_ptr=None), "in_device is null"), (dict(out_ptr=None), "out_device is null"),
            (dict(in_ptr=src.ptr + 2), "in_device is not a multiple of 4 bytes"), (dict(out_ptr=out.ptr + 1), "out_device is not a multiple of 4 bytes"),
            (dict(in_ptr=host.ctypes.data), "in_device is not device memory"), (dict(out_ptr=host.ctypes.data), "out_device is not device memory"),
        ]
        for kw, text in bad:
            args = dict(in_ptr=src.ptr, out_ptr=out.ptr, n=8, mode=v.PATH_CONSECUTIVE, sigma=1.5, min_peak=0.0)
            args.update(kw)
            with pytest.raises(v.FftupError) as e:
                v.shift_path(**args)
            assert e.value.code == 1 and text in str(e.value), (kw, str(e.value))
        lib = v._lib.load()
        assert lib.fftup_shift_path(None, src.ptr, out.ptr, 8, None) == 1 and b"cfg is null" in lib.fftup_last_error()
        assert out.untouched() and not host.any()
        assert src.read()[0].tobytes() == sh.tobytes()
        # ... and the call still works
        v.shift_path(src.ptr, out.ptr, 8, v.PATH_CONSECUTIVE, 1.5, 0.0)
        got, ok = out.read()
        assert ok and (np.abs(got[:, :2].astype(np.float64) - PO.path(sh, PO.CONSECUTIVE, 1.5, 0.0)[2]) <= PO.out_bar(PO.path(sh, PO.CONSECUTIVE, 1.5, 0.0)[2])).all()
    finally:
        src.close()
        out.close()


# ---------------------------------------------------------------- 6. the command-line tool
def _cli_clip(tmp_path):
    shifts = [(0.0, 0.0)] + STAB_SHIFTS[:3]
    frames = AO.clip(SW, SH, 1, shifts, seed=5)
    src = tmp_path / "in"
    src.mkdir()
    for k, f in enumerate(frames):
        P.png_write(str(src / ("%06d.png" % (k + 1))), f)
    return frames, src


def _cli_args(src, dst):
    return [CLI, "-stabilise", "-ifolder", str(src), "-ofolder", str(dst), "-numfiles", "4", "-size", "%dx%d" % (SUW, SUH), "-view", "4,2,40,36", "-s", "0"]


def test_cli_stabilise_renders_the_bytes_of_the_host_chain(tmp_path):
    """-stabilise without new flags: the files are, by bytes, the RGB8 outputs of execute_device_views fed stabilised_views of
    Aligner.shifts -- the shifts now reach the views through device memory, the pictures are the ones of the host loop"""
    import vkresample_amd as v
    frames, src = _cli_clip(tmp_path)
    dst = tmp_path / "out"
    dst.mkdir()
    ims = [Image(RGB8, SW, SH, 1, frame=f) for f in frames]
    try:
        with v.Aligner(SW, SH) as al:
            est = al.shifts(ims[0].image, [im.image for im in ims])
    finally:
        for im in ims:
            im.close()
    r = subprocess.run(_cli_args(src, dst), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^frame (\d{6}): shift (-?\d+\.\d{3}) (-?\d+\.\d{3}) peak (-?\d+\.\d{3})$", r.stdout, re.M)
    assert [l[0] for l in lines] == ["%06d" % (k + 1) for k in range(4)], r.stdout
    assert "offset" not in r.stdout
    for l, e in zip(lines, est):
        assert abs(float(l[1]) - e[0]) <= 0.0005 + 2.0 ** -23 * max(abs(e[0]), 1) and abs(float(l[2]) - e[1]) <= 0.0005 + 2.0 ** -23 * max(abs(e[1]), 1), (l, e)
    with v.Upscaler.view(SW, SH, SUW, SUH, STAB_VIEW[0], STAB_VIEW[1], sharpen=0.0) as up:
        want, _ = _run(up, frames, RGB8, v.stabilised_views(STAB_VIEW, est), None, RGB8)
    assert sorted(os.listdir(dst)) == ["%06d.png" % (k + 1) for k in range(4)]
    for k in range(4):
        assert np.array_equal(P.png_read(str(dst / ("%06d.png" % (k + 1)))), want[k].reshape(SUH, SUW, 3)), k


def test_cli_smooth(tmp_path):
    """-smooth 1.5: the pairs are consecutive frames; the printed offsets are path_oracle's on the device's estimates (re-measured
    here), within the printed precision 0.0005 + one fp32 rounding step; the files are the shifted call's bytes; the bad invocations
    print one line, exit 1 and write nothing"""
    import vkresample_amd as v
    frames, src = _cli_clip(tmp_path)
    dst = tmp_path / "out"
    dst.mkdir()
    ims = [Image(RGB8, SW, SH, 1, frame=f) for f in frames]
    try:
        d = [im.image for im in ims]
        with v.Aligner(SW, SH) as al, v.DeviceBuffer(16 * 4) as est_buf, v.DeviceBuffer(16 * 4) as off_buf, \
                v.Upscaler.view(SW, SH, SUW, SUH, STAB_VIEW[0], STAB_VIEW[1], sharpen=0.0) as up:
            al.shifts_device([d[0]] + d[:-1], d, est_buf.ptr)
            v.shift_path(est_buf.ptr, off_buf.ptr, 4, v.PATH_CONSECUTIVE, 1.5, 0.0)
            est = est_buf.download().view(np.float32).reshape(4, 4).copy()
            off = off_buf.download().view(np.float32).reshape(4, 4).copy()
            outs = [Image(RGB8, SUW, SUH, 1) for _ in frames]
            try:
                up.execute_device_views_shifted(d, [o.image for o in outs], [STAB_VIEW] * 4, off_buf.ptr)
                want = [o.read()[0] for o in outs]
            finally:
                for o in outs:
                    o.close()
    finally:
        for im in ims:
            im.close()
    oracle = PO.path(est, PO.CONSECUTIVE, 1.5, 0.0)[2]
    assert (np.abs(off[:, :2].astype(np.float64) - oracle) <= PO.out_bar(oracle)).all() and np.abs(oracle).max() > 0.5
    r = subprocess.run(_cli_args(src, dst) + ["-smooth", "1.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^frame (\d{6}): shift (-?\d+\.\d{3}) (-?\d+\.\d{3}) peak (-?\d+\.\d{3}) offset (-?\d+\.\d{3}) (-?\d+\.\d{3})$", r.stdout, re.M)
    assert [l[0] for l in lines] == ["%06d" % (k + 1) for k in range(4)], r.stdout
    for k, l in enumerate(lines):
        for a in (0, 1):
            assert abs(float(l[1 + a]) - est[k, a]) <= 0.0005 + 2.0 ** -23 * max(abs(est[k, a]), 1), (l, est[k])
            assert abs(float(l[4 + a]) - oracle[k, a]) <= 0.0005 + PO.out_bar(oracle)[k, a], (l, oracle[k])
    assert sorted(os.listdir(dst)) == ["%06d.png" % (k + 1) for k in range(4)]
    for k in range(4):
        assert np.array_equal(P.png_read(str(dst / ("%06d.png" % (k + 1)))), want[k].reshape(SUH, SUW, 3)), k
    bad_dst = tmp_path / "bad"
    bad_dst.mkdir()
    plain = [CLI, "-ifolder", str(src), "-ofolder", str(bad_dst), "-numfiles", "4", "-size", "%dx%d" % (SUW, SUH), "-view", "4,2,40,36", "-s", "0"]
    for args in (plain + ["-smooth", "1.5"], _cli_args(src, bad_dst) + ["-smooth", "-1"], _cli_args(src, bad_dst) + ["-smooth", "wide"],
                 _cli_args(src, bad_dst) + ["-smooth"], _cli_args(src, bad_dst) + ["-minpeak", "0.5"], _cli_args(src, bad_dst) + ["-smooth", "1.5", "-minpeak", "x"]):
        r = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and len(r.stdout.strip().splitlines()) == 1 and not os.listdir(bad_dst), (args, r.stdout)
    # -minpeak above every peak: no frame is trusted, the path holds at 0 and every offset is 0
    r = subprocess.run(_cli_args(src, bad_dst) + ["-smooth", "1.5", "-minpeak", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and len(re.findall(r" offset -?0\.000 -?0\.000$", r.stdout, re.M)) == 4, r.stdout
