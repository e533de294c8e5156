"""GPU: fftup_align_shifts (Aligner) -- phase-correlation shift estimates of frame pairs in device memory.

The yardstick is tests/align_oracle.py, the estimate restated in fp64 numpy, on 8-bit synthetic clips (float and half planes are
conversions of the 8-bit frames): computed once per case and input format, shared and left unchanged.

Bars.  dx, dy: one fine cell, d / kappa -- the most a flipped near-tie of the fine argmax can move a parabola's vertex -- and the same
coarse cell, after the ORACLE's best and second-best coarse values were seen to differ by more than 1e-3 (otherwise the argmax is a
coin toss).  peak, peak_coarse: the oracle run in complex64 and in complex128 over these cases and formats on the CPU differs by at
most 2.4e-7 (the 80 x 48 case, half planes); four times that, PEAK_BAR = 9.6e-7, is allowed.  The coarse cell itself is not
part of a fftup_shift: it is the same when peak_coarse agrees within PEAK_BAR, since no other cell of the oracle comes within 1e-3 of
the best one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import align_oracle as AO
from devimage import FILL, GUARD, PLANAR, RGB8, Image
from paritylib import CLI, measured, png_read, png_write, rel_l2

pytestmark = pytest.mark.gpu

KAPPA = 32
PEAK_BAR = 4 * 2.4e-7
# name -> (descriptor format, precision of the aligner, bytes per element, conversion of an 8-bit frame)
FORMATS = {"rgb8": (RGB8, 0, 1, lambda f: f),
           "planar_f32": (PLANAR, 0, 4, lambda f: AO.planes_of(f, np.float32)),
           "planar_f16": (PLANAR, 2, 2, lambda f: AO.planes_of(f, np.float16))}
GPU_CASES = AO.CASES + [AO.WIDE_CASE]
CASE_IDS = ["%dx%d_w%dx%d_d%d" % (c[0], c[1], c[2][0], c[2][1], c[3]) for c in GPU_CASES]

_clips, _oracles = {}, {}


def _clip(case):
    if case not in _clips:
        W, H, _, d = case
        ref, moved, true = AO.case_clip(W, H, d)
        for f in [ref] + moved:
            f.flags.writeable = False
        _clips[case] = (ref, moved, true)
    return _clips[case]


def _oracle(case, fmt):
    """the fp64 estimates of the case's pairs on the values the library reads in this format: computed once"""
    if (case, fmt) not in _oracles:
        W, H, window, d = case
        conv = FORMATS[fmt][3]
        ref, moved, _ = _clip(case)
        g = AO.geometry(W, H, window, d)
        _oracles[(case, fmt)] = [AO.estimate(conv(ref), conv(cur), g) for cur in moved]
    return _oracles[(case, fmt)]


def _images(case, fmt, frames, padded=False, base=GUARD):
    W, H = case[0], case[1]
    dfmt, _, esz, conv = FORMATS[fmt]
    return [Image(dfmt, W, H, esz, padded, base, conv(f)) for f in frames]


def _aligner(case, fmt, **kw):
    import vkresample_amd as v
    W, H, window, d = case
    return v.Aligner(W, H, FORMATS[fmt][1], window=window, decimate=d, **kw)


def _close(images):
    for im in images:
        im.close()


# ---------------------------------------------------------------- 1. parity with the oracle
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("case", GPU_CASES, ids=CASE_IDS)
def test_parity_with_the_oracle(case, fmt):
    """seven pairs in one call with max_batch = 3: chunks of 3, 3 and 1, the buffers reused in stream order.
    Bars: |dx|, |dy| within d / kappa of the oracle; peak and peak_coarse within PEAK_BAR = 9.6e-7, four times the 2.4e-7 by which
    the oracle in complex64 differs from the oracle in complex128 over these cases.  Measured on an MI355X, all four cases and three
    formats: dx, dy within 8.2e-6 pixels, peak within 4.8e-7, peak_coarse within 5.4e-7.
    The 600 x 300 case runs the list's shifts with the half-pixel components at quarter pixels (tests/align_oracle.py, WIDE_SHIFTS, has
    the reason: at 512 x 256 a half-pixel shift leaves the oracle's two best cells 4e-4 apart with every clip seed); the half-pixel
    shifts at that window have the next test to themselves."""
    d = case[3]
    ref, moved, true = _clip(case)
    moved, oracle = moved[:7], _oracle(case, fmt)[:7]
    ims = _images(case, fmt, [ref] + moved)
    try:
        with _aligner(case, fmt, max_batch=3) as al:
            assert al.info["upsample"] == KAPPA and (al.info["window_w"], al.info["window_h"], al.info["decimate"]) == (case[2][0], case[2][1], d)
            got = al.shifts(ims[0].image, [im.image for im in ims[1:]])
    finally:
        _close(ims)
    assert got.shape == (7, 4) and got.dtype == np.float32
    for k, (g, o) in enumerate(zip(got, oracle)):
        measured("align %s %s pair %d" % (CASE_IDS[GPU_CASES.index(case)], fmt, k), ddx=abs(g[0] - o["dx"]), ddy=abs(g[1] - o["dy"]),
                 dpeak=abs(g[2] - o["peak"]), dcoarse=abs(g[3] - o["peak_coarse"]), oracle_gap=o["gap"], true_dx=true[k][0], got_dx=g[0])
    for k, o in enumerate(oracle):
        assert o["gap"] > 1e-3, "pair %d: the oracle's coarse argmax is a coin toss (gap %.3g)" % (k, o["gap"])
    for k, (g, o) in enumerate(zip(got, oracle)):
        assert abs(g[3] - o["peak_coarse"]) <= PEAK_BAR, (k, g, o)            # ... which also says: the same coarse cell
        assert abs(g[0] - o["dx"]) <= d / KAPPA and abs(g[1] - o["dy"]) <= d / KAPPA, (k, g, o)
        assert abs(g[2] - o["peak"]) <= PEAK_BAR, (k, g, o)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_half_pixel_shifts_on_the_wide_window(fmt):
    """(3.25, -1.5) and (-0.5, -0.5) at 600 x 300 with a 512 x 256 window: the oracle's best coarse cells are 4.4e-4 and 4.3e-4 apart,
    so either may win.  peak_coarse has to be the oracle's value of ONE of its cells within 1e-3 of the best, within PEAK_BAR; dx, dy
    and peak have the bars of the parity test -- the fine grid reaches a whole pixel to each side, so both cells lead to the same
    fine maximum.  (Measured: the library picks the oracle's cell; dx, dy within 8.2e-6 pixels, peak_coarse within 1.2e-7.)"""
    case = AO.WIDE_CASE
    ref, moved, true = _clip(case)
    moved, true, oracle = moved[7:], true[7:], _oracle(case, fmt)[7:]
    assert len(moved) == 2 and all(len(o["near"]) >= 2 or o["gap"] > 1e-3 for o in oracle)
    ims = _images(case, fmt, [ref] + moved)
    try:
        with _aligner(case, fmt) as al:
            got = al.shifts(ims[0].image, [im.image for im in ims[1:]])
    finally:
        _close(ims)
    for k, (g, o) in enumerate(zip(got, oracle)):
        dcoarse = min(abs(g[3] - v) for v in o["near"])
        measured("align wide half-pixel %s pair %d" % (fmt, k), ddx=abs(g[0] - o["dx"]), ddy=abs(g[1] - o["dy"]), dpeak=abs(g[2] - o["peak"]),
                 dcoarse=dcoarse, oracle_gap=o["gap"], true_dx=true[k][0], got_dx=g[0])
        assert dcoarse <= PEAK_BAR, (k, g, o)
        assert abs(g[0] - o["dx"]) <= 1 / KAPPA and abs(g[1] - o["dy"]) <= 1 / KAPPA, (k, g, o)
        assert abs(g[2] - o["peak"]) <= PEAK_BAR, (k, g, o)


# ---------------------------------------------------------------- 2. identical frames
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_identical_frames(fmt):
    """a frame against itself (the same descriptor) and against a second copy of it in other memory: dx = dy = 0 exactly, peak 1"""
    case = GPU_CASES[0]
    ref = _clip(case)[0]
    ims = _images(case, fmt, [ref, ref])
    try:
        with _aligner(case, fmt) as al:
            got = al.shifts([ims[0].image, ims[0].image], [ims[0].image, ims[1].image])
    finally:
        _close(ims)
    for g in got:
        measured("align identical %s" % fmt, dx=g[0], dy=g[1], dpeak=abs(g[2] - 1.0), dcoarse=abs(g[3] - 1.0))
    for g in got:
        assert g[0] == 0.0 and g[1] == 0.0, got
        assert abs(g[2] - 1.0) <= PEAK_BAR and abs(g[3] - 1.0) <= PEAK_BAR, got


# ---------------------------------------------------------------- 3. aliasing
def test_aliased_descriptors_give_the_results_of_separate_calls():
    """consecutive frames (cur[i] is also ref[i + 1]) and a fixed reference (one descriptor repeated), each in ONE call, against
    one call per pair: bit for bit"""
    case = GPU_CASES[0]
    ref, moved, _ = _clip(case)
    ims = _images(case, "rgb8", [ref] + moved[:4])
    try:
        with _aligner(case, "rgb8") as al:
            d = [im.image for im in ims]
            chain = al.shifts(d[:-1], d[1:])
            fixed = al.shifts([d[0]] * 4, d[1:])
            chain_1 = np.concatenate([al.shifts([d[k]], [d[k + 1]]) for k in range(4)])
            fixed_1 = np.concatenate([al.shifts([d[0]], [d[k + 1]]) for k in range(4)])
    finally:
        _close(ims)
    assert chain.tobytes() == chain_1.tobytes() and fixed.tobytes() == fixed_1.tobytes()
    assert np.abs(chain[:, :2]).max() > 0.5                   # (the frames did move)


# ---------------------------------------------------------------- 4. containment and ordering
class _Result:
    """n fftup_shift in device memory between two guard bands of 0xA5"""

    def __init__(self, n):
        import vkresample_amd as v
        self.n = n
        self.buf = v.DeviceBuffer(2 * GUARD + 16 * n)
        self.buf.upload(np.full(2 * GUARD + 16 * n, FILL, np.uint8))
        self.ptr = self.buf.ptr + GUARD

    def read(self, stream=None):
        """-> ((n, 4) float32, True if both guard bands are untouched)"""
        raw = self.buf.download(stream=stream)
        body = raw[GUARD:GUARD + 16 * self.n]
        return body.view(np.float32).reshape(self.n, 4).copy(), bool((raw[:GUARD] == FILL).all() and (raw[GUARD + 16 * self.n:] == FILL).all())

    def untouched(self):
        return bool((self.buf.download() == FILL).all())

    def close(self):
        self.buf.close()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_guards_strides_and_streams(fmt):
    """dense frames, then rows and planes with padding (8-bit rows at an odd byte address): the same results bit for bit, every guard
    byte and every byte of padding untouched, the frames unchanged; then the call on a stream of its own, read back on that stream"""
    import vkresample_amd as v
    case = GPU_CASES[0]
    ref, moved, _ = _clip(case)
    frames = [ref] + moved[:3]
    dense = _images(case, fmt, frames)
    padded = _images(case, fmt, frames, padded=True, base=GUARD + (1 if fmt == "rgb8" else 0))
    res = [_Result(3) for _ in range(3)]
    try:
        with _aligner(case, fmt) as al, v.Stream() as s:
            al.shifts_device(dense[0].image, [im.image for im in dense[1:]], res[0].ptr)
            al.shifts_device(padded[0].image, [im.image for im in padded[1:]], res[1].ptr)
            a, a_ok = res[0].read()
            b, b_ok = res[1].read()
            al.shifts_device(dense[0].image, [im.image for im in dense[1:]], res[2].ptr, stream=s)
            c, c_ok = res[2].read(stream=s)
        assert a_ok and b_ok and c_ok
        assert a.tobytes() == b.tobytes() == c.tobytes() and np.abs(a[:, :2]).max() > 0.5
        conv = FORMATS[fmt][3]
        for group in (dense, padded):
            for im, f in zip(group, frames):
                pixels, guards = im.read()
                assert guards and pixels.tobytes() == np.ascontiguousarray(conv(f)).tobytes()
    finally:
        _close(dense + padded + res)


# ---------------------------------------------------------------- 5. validation
def test_invalid_calls_are_refused_before_any_launch():
    import vkresample_amd as v
    from vkresample_amd import _lib
    case = GPU_CASES[0]
    W, H = case[0], case[1]
    ref, moved, _ = _clip(case)
    ims = _images(case, "rgb8", [ref, moved[1]])
    res = _Result(2)
    host = np.zeros((H, W, 3), np.uint8)
    try:
        with _aligner(case, "rgb8") as al:
            good = ims[0].image
            bad = [
                ([v.DeviceImage(host.ctypes.data, RGB8, 3 * W)], [ims[1].image], res.ptr, r"ref\[0\]\.data is not device memory"),
                ([good], [v.DeviceImage(ims[1].image.ptr, RGB8, 3 * W - 1)], res.ptr, r"cur\[0\]\.row_stride_bytes \d+ is below one row"),
                ([good], [v.DeviceImage(ims[1].image.ptr, 7, 3 * W)], res.ptr, r"cur\[0\]\.format 7 is not a FFTUP_FMT_\* format"),
                ([good], [ims[1].image], None, r"shifts_device is null"),
                ([good], [ims[1].image], host.ctypes.data, r"shifts_device is not device memory"),
            ]
            for refs, curs, out, text in bad:
                with pytest.raises(v.FftupError) as e:
                    al.shifts_device(refs, curs, out)
                assert e.value.code == 1 and re.search(text, str(e.value)), str(e.value)
            a = (_lib.DeviceImageDesc * 1)(good.desc())
            assert al._lib.fftup_align_shifts(al._h, a, a, 0, res.ptr, None) == 1 and "n_pairs must be > 0" in al._lib.fftup_last_error().decode()
            assert al._lib.fftup_align_shifts(al._h, None, a, 1, res.ptr, None) == 1 and "null image array" in al._lib.fftup_last_error().decode()
            assert res.untouched()                       # nothing was enqueued: the blocking read-back finds every byte as it was
            # ... and the aligner still works
            al.shifts_device([good, good], [ims[1].image, ims[1].image], res.ptr)
            got, ok = res.read()
            assert ok and got[0].tobytes() == got[1].tobytes() and abs(got[0][0]) > 0.5
    finally:
        _close(ims + [res])


# ---------------------------------------------------------------- 6. stabilisation end to end
SW, SH, SUW, SUH = 48, 40, 40, 36
STAB_SHIFTS = [(1.3, -0.7), (-2.2, 1.6), (2.75, 2.1), (-0.9, -2.6), (3.0, 0.4)]
STAB_VIEW = ((4.0, 2.0), (40.0, 36.0))


def _render(up, images, views):
    outs = [Image(PLANAR, SUW, SUH, 4) for _ in images]
    try:
        up.execute_device_views([im.image for im in images], [o.image for o in outs], views)
        return [o.read()[0].view(np.float32).astype(np.float64) for o in outs]
    finally:
        _close(outs)


def test_stabilised_clip_end_to_end():
    """a reference and five frames moved by known amounts of at most 3 px, each moved frame rendered by a periodic view plan at the
    view's origin + shift, the shift taken from the GPU's estimates (G), the oracle's (O) and the truth (T): per frame
    rel_l2(G, T) <= 2 rel_l2(O, T) + 1e-6 -- the reference chain sets the bar, with a margin of 2 for fp32 -- and the clip did move:
    rel_l2(T, the frame rendered at the plain view) > 10 rel_l2(G, T)"""
    import vkresample_amd as v
    frames = AO.clip(SW, SH, 1, [(0.0, 0.0)] + STAB_SHIFTS, seed=5)
    g = AO.geometry(SW, SH)
    oracle = [AO.estimate(frames[0], f, g) for f in frames[1:]]
    ims = [Image(RGB8, SW, SH, 1, frame=f) for f in frames]
    try:
        with v.Aligner(SW, SH) as al:
            assert (al.info["window_w"], al.info["window_h"], al.info["decimate"]) == (g["nx"], g["ny"], g["d"]) == (32, 32, 1)
            est = al.shifts(ims[0].image, [im.image for im in ims[1:]])
        with v.Upscaler.view(SW, SH, SUW, SUH, STAB_VIEW[0], STAB_VIEW[1], sharpen=0.0) as up:
            moved = ims[1:]
            G = _render(up, moved, v.stabilised_views(STAB_VIEW, est))
            Oo = _render(up, moved, v.stabilised_views(STAB_VIEW, [(o["dx"], o["dy"]) for o in oracle]))
            T = _render(up, moved, v.stabilised_views(STAB_VIEW, STAB_SHIFTS))
            U = _render(up, moved, [STAB_VIEW] * len(moved))
    finally:
        _close(ims)
    figures = []
    for k in range(len(STAB_SHIFTS)):
        gt, ot, ut = rel_l2(G[k], T[k]), rel_l2(Oo[k], T[k]), rel_l2(U[k], T[k])
        measured("stabilise frame %d" % k, rel_G_T=gt, rel_O_T=ot, rel_unstabilised_T=ut, dx=est[k][0], dy=est[k][1], oracle_dx=oracle[k]["dx"], oracle_dy=oracle[k]["dy"])
        figures.append((gt, ot, ut))
    for gt, ot, ut in figures:
        assert gt <= 2 * ot + 1e-6, figures
        assert ut > 10 * gt, figures


# ---------------------------------------------------------------- 7. the command-line tool
def test_cli_stabilise(tmp_path):
    import vkresample_amd as v
    shifts = [(0.0, 0.0)] + STAB_SHIFTS[:3]
    frames = AO.clip(SW, SH, 1, shifts, seed=5)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    for k, f in enumerate(frames):
        png_write(str(src / ("%06d.png" % (k + 1))), f)
    ims = [Image(RGB8, SW, SH, 1, frame=f) for f in frames]
    try:
        with v.Aligner(SW, SH) as al:
            est = al.shifts(ims[0].image, [im.image for im in ims])
    finally:
        _close(ims)
    args = [CLI, "-stabilise", "-ifolder", str(src), "-ofolder", str(dst), "-numfiles", "4", "-size", "%dx%d" % (SUW, SUH),
            "-view", "4,2,40,36", "-s", "0"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^frame (\d{6}): shift (-?\d+\.\d{3}) (-?\d+\.\d{3}) peak (-?\d+\.\d{3})$", r.stdout, re.M)
    assert [l[0] for l in lines] == ["%06d" % (k + 1) for k in range(4)], r.stdout
    for l, e in zip(lines, est):
        assert abs(float(l[1]) - e[0]) <= 1 / KAPPA + 0.0005 and abs(float(l[2]) - e[1]) <= 1 / KAPPA + 0.0005, (l, e)
    written = sorted(os.listdir(dst))
    assert written == ["%06d.png" % (k + 1) for k in range(4)]
    assert png_read(str(dst / written[0])).shape == (SUH, SUW, 3)
    for extra, text in ((["-numthreads", "2"], "-numthreads above 1"), (["-gpupng"], "-gpupng")):
        r = subprocess.run(args + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and text in r.stdout and len(r.stdout.strip().splitlines()) == 1, r.stdout
    r = subprocess.run([CLI, "-stabilise", "-ifolder", str(src), "-ofolder", str(dst), "-numfiles", "4", "-u", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "-stabilise needs an output size given with -size" in r.stdout
    r = subprocess.run([CLI, "-stabilise", "-i", str(src / "000001.png"), "-size", "40x36"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "cannot be combined with -i" in r.stdout
