"""GPU: the rotator (fftup_rotate_*, include/fftup.h: rotation by three Fourier shears) against its fp64 oracle
(tests/rotate_oracle.py, itself held to known answers by tests/test_rotate_oracle.py), on images in caller-owned device memory with
guard bands and padding (tests/devimage.py).  Shapes, frames, rotations and bars: tests/rotate_cases.py -- the fp32 bars are four
times the difference between the oracle in complex64 and in complex128 over exactly these frames, measured on the CPU
(max |difference| 6.31e-7 -> FP32_ABS = 2.56e-6; relative L2 2.03e-7 -> FP32_REL_L2 = 8.4e-7), and tests/test_rotate_bars.py keeps
the recorded figures honest.

Measured on an MI355X, all seven shapes, seven frames each (pytest -s prints every figure):
    float planes -> float planes   max |difference| <= 9.03e-7, relative L2 <= 2.44e-7
    8-bit -> float planes          max |difference| <= 7.94e-7, relative L2 <= 2.61e-7
    half planes -> half planes     every value within one binary16 step of the oracle's rounding (0.999 of the bound, as the
                                   complex64 oracle's own rounding; 0.42 % of a frame's values differ at most)
    8-bit -> 8-bit                 at most 0.0132 % of a frame's codes differ from the oracle's, each by 1 and at a near-tie
    theta = 0, float planes        max |difference| <= 7.15e-7; 8-bit: byte for byte
    theta then -theta, odd sizes   max |difference| <= 8.34e-7 (bar 5.12e-6)
    the Gaussian of 96 x 80        max |difference| to the analytic rotation <= 4.35e-7; the opposite sign is off by 0.507 and more
"""
import subprocess

import numpy as np
import pytest

import devimage as D
import paritylib as P
import rotate_cases as K
import rotate_oracle as R

pytestmark = pytest.mark.gpu

# (input kind, output kind, the rotator's precision)
FORMATS = [("f32", "f32", 0), ("u8", "f32", 0), ("f16", "f16", 2), ("u8", "u8", 0)]
NP = {"f32": np.float32, "f16": np.float16}


def host_frame(kind, rgb):
    """what a frame of 8-bit codes is in memory as `kind`"""
    return rgb if kind == "u8" else R.planes_of(rgb).astype(NP[kind])


def decode(kind, raw, W, H):
    """the pixels' bytes -> codes [H, W, 3] or values [3, H, W] float64"""
    if kind == "u8":
        return raw.reshape(H, W, 3)
    return raw.view(NP[kind]).reshape(3, H, W).astype(np.float64)


def image(kind, precision, W, H, frame=None, padded=False, odd_base=False):
    fmt = D.RGB8 if kind == "u8" else D.PLANAR
    return D.Image(fmt, W, H, D.ESZ[precision], padded, D.GUARD + (1 if odd_base and kind != "u8" else 0), frame)


def run(W, H, fin, fout, precision, frames, rots, max_batch=0, stream=None, in_place=False, varied=True):
    """one fftup_rotate_frames call -> per frame (the output pixels' bytes, every other byte of its buffer still 0xA5, the input
    buffer byte for byte what was uploaded).  varied: frames alternate between dense and padded layouts, input 2 and output 4 sit at
    an odd address (planes); otherwise every image is padded."""
    import vkresample_amd as v
    n = len(frames)
    src = [image(fin, precision, W, H, host_frame(fin, f), (i % 2 == 1) if varied else True, varied and i == 2) for i, f in enumerate(frames)]
    dst = src if in_place else [image(fout, precision, W, H, None, (i % 2 == 0) if varied else True, varied and i == 4) for i in range(n)]
    try:
        before = [s.buf.download() for s in src]
        with v.Rotator(W, H, precision, 0, max_batch) as rot:
            rot.rotate([s.image for s in src], [d.image for d in dst], list(rots), stream)
            out = [d.read(stream) for d in dst]
            same = [bool((s.buf.download(stream=stream) == b).all()) for s, b in zip(src, before)]
        return [(o[0], o[1], k) for o, k in zip(out, same)]
    finally:
        for im in src + ([] if in_place else dst):
            im.close()


def check_u8(tag, got, ox):
    """8-bit output against the oracle's values ox: a code may differ from the oracle's only by 1, and only at a near-tie"""
    want = R.to_u8(ox)
    tie = K.near_tie(ox)
    diff = got.astype(np.int32) - want.astype(np.int32)
    P.measured(tag, near_tie_share=tie.mean(), differing_share=(diff != 0).mean(), max_code_diff=np.abs(diff).max())
    assert np.abs(diff).max() <= 1
    assert not ((diff != 0) & ~tie).any()


@pytest.mark.parametrize("fmt", FORMATS, ids=["%s-%s" % f[:2] for f in FORMATS])
@pytest.mark.parametrize("size", R.CASES, ids=["%dx%d" % s for s in R.CASES])
def test_parity_with_the_oracle(size, fmt):
    """Seven frames in ONE call on a rotator with max_batch = 3 (chunks of 3, 3 and 1, the intermediates reused in stream order),
    dense and padded layouts, one input and one output at an odd address.  Bars: float planes FP32_ABS = 2.56e-6 and
    FP32_REL_L2 = 8.4e-7, four times the complex64 oracle's 6.31e-7 and 2.03e-7 (tests/rotate_cases.py); half planes one binary16
    step of the oracle's rounding (paritylib); 8-bit: a differing code differs by 1 and sits where the oracle's 255 x + 0.5 lies
    within 255 FP32_ABS of an integer, and such near-ties are below 1 % of every frame of the ORACLE (a cap that keeps the test
    honest, asserted first; the oracle's share is at most 2.3e-3).  Measured on an MI355X: float planes at most 9.03e-7 and 2.61e-7;
    half planes at most 0.999 of the bound; 8-bit at most 0.0132 % of a frame's codes differ."""
    W, H = size
    fin, fout, precision = fmt
    ox = K.oracle(W, H, fin)
    if fout == "u8":
        for x in ox:
            assert K.near_tie(x).mean() <= K.NEAR_TIE_CAP
    res = run(W, H, fin, fout, precision, K.frames_u8(W, H), K.rotations(W, H), max_batch=3)
    for i, ((raw, clean, same), x) in enumerate(zip(res, ox)):
        tag = "rotate %dx%d %s->%s frame %d" % (W, H, fin, fout, i)
        assert clean, tag + ": a byte outside the named pixels was written"
        assert same, tag + ": the input was written"
        got = decode(fout, raw, W, H)
        if fout == "u8":
            check_u8(tag, got, np.transpose(x, (1, 2, 0)))
        elif fout == "f32":
            P.measured(tag, max_abs=np.abs(got - x).max(), rel_l2=P.rel_l2(got, x))
            assert np.abs(got - x).max() <= K.FP32_ABS
            assert P.rel_l2(got, x) <= K.FP32_REL_L2
        else:
            o16 = x.astype(np.float16).astype(np.float64)
            P.measured(tag, worst_share_of_bound=(np.abs(got - o16) / P.one_half_ulp_bound(o16)).max(), differing=(got != o16).mean())
            assert P.within_one_half_ulp(got, o16).all()


@pytest.mark.parametrize("size", R.CASES, ids=["%dx%d" % s for s in R.CASES])
def test_zero_angle(size):
    """theta = 0: every phase is exactly (1, 0), so 8-bit -> 8-bit is byte for byte the input (round to nearest: what the
    transforms' rounding leaves is far below half a code) and float planes come back within FP32_ABS (measured: 7.15e-7 at most)"""
    W, H = size
    rgb = K.frames_u8(W, H)[0]
    (raw, clean, same), = run(W, H, "u8", "u8", 0, [rgb], [0.0])
    assert clean and same
    assert (decode("u8", raw, W, H) == rgb).all()
    (raw, clean, same), = run(W, H, "f32", "f32", 0, [rgb], [0.0])
    x = R.planes_of(rgb).astype(np.float32).astype(np.float64)
    err = np.abs(decode("f32", raw, W, H) - x).max()
    P.measured("rotate %dx%d theta 0" % (W, H), max_abs=err)
    assert clean and same and err <= K.FP32_ABS


@pytest.mark.parametrize("size", [(45, 21), (75, 45)], ids=["45x21", "75x45"])
def test_round_trip_on_odd_sizes(size):
    """theta, then -theta through a second call: on odd x odd frames every shear is a unitary phase ramp, so the input comes back --
    within twice FP32_ABS (two rotations; 5.12e-6), whatever the oracle says.  Measured on an MI355X: at most 8.34e-7."""
    W, H = size
    thetas = [0.02, -0.3, 0.7, 1.5]
    rgb = [R.noise_u8(W, H, 40 + i) for i in range(len(thetas))]
    there = run(W, H, "f32", "f32", 0, rgb, thetas)
    mid = [decode("f32", r[0], W, H) for r in there]
    import vkresample_amd as v
    src = [image("f32", 0, W, H, m.astype(np.float32)) for m in mid]
    dst = [image("f32", 0, W, H) for _ in mid]
    try:
        with v.Rotator(W, H) as rot:
            rot.rotate([s.image for s in src], [d.image for d in dst], [-t for t in thetas])
            back = [decode("f32", d.read()[0], W, H) for d in dst]
    finally:
        for im in src + dst:
            im.close()
    for t, f, b, m in zip(thetas, rgb, back, mid):
        x = R.planes_of(f).astype(np.float32).astype(np.float64)
        err = np.abs(b - x).max()
        P.measured("rotate round trip %dx%d theta %+.2f" % (W, H, t), max_abs=err, moved=np.abs(m - x).max())
        assert err <= 2 * K.FP32_ABS
        assert np.abs(m - x).max() > 0.1                      # (the frame in between is another image)


def test_known_answer_gaussian():
    """the Gaussian of tests/test_rotate_oracle.py at 96 x 80 matches its analytic rotation within FP32_ABS (the oracle's own
    distance to it is 4e-9) and the wrong sign is off by more than 0.5: direction and centre, without the oracle.  Measured: 4.35e-7."""
    W, H = 96, 80
    c = R.centre_of(W, H)
    thetas = [0.1, -0.4, 0.9]
    import vkresample_amd as v
    g = np.repeat(R.gaussian(W, H, c)[None], 3, axis=0).astype(np.float32)
    src = image("f32", 0, W, H, g)
    dst = [image("f32", 0, W, H) for _ in thetas]
    try:
        with v.Rotator(W, H) as rot:
            rot.rotate([src.image] * 3, [d.image for d in dst], thetas)
            got = [decode("f32", d.read()[0], W, H) for d in dst]
    finally:
        for im in [src] + dst:
            im.close()
    for t, y in zip(thetas, got):
        err = np.abs(y - R.gaussian(W, H, c, angle=t)[None]).max()
        wrong = np.abs(y - R.gaussian(W, H, c, angle=-t)[None]).max()
        P.measured("rotate gaussian theta %+.1f" % t, max_abs=err, opposite_sign=wrong)
        assert err <= K.FP32_ABS and wrong > 0.5


@pytest.mark.parametrize("kind,precision", [("u8", 0), ("f32", 0), ("f16", 2)])
def test_in_place_and_containment(kind, precision):
    """out[i] == in[i] gives the bytes of the out-of-place call; every byte outside the named pixels of the padded images is still
    0xA5; the inputs of the out-of-place call are unchanged"""
    W, H = 60, 42
    frames, rots = K.frames_u8(W, H)[:4], K.rotations(W, H)[1:5]
    apart = run(W, H, kind, kind, precision, frames, rots, max_batch=3, varied=False)
    inpl = run(W, H, kind, kind, precision, frames, rots, max_batch=3, varied=False, in_place=True)
    for (raw, clean, same), (raw2, clean2, _) in zip(apart, inpl):
        assert clean and same and clean2
        assert (raw == raw2).all()
    assert not (apart[0][0] == host_frame(kind, frames[0]).reshape(-1).view(np.uint8)).all()


def test_ordering_on_a_callers_stream():
    """a rotation enqueued on a caller's stream behind the copy of its input and ahead of the copy of its output gives the right
    bytes with no host wait in between; two calls back to back on ONE rotator (max_batch = 1: the same intermediates) with different
    angles each give their own result"""
    import vkresample_amd as v
    W, H = 96, 80
    rgb = K.frames_u8(W, H)[0]
    want = [run(W, H, "u8", "u8", 0, [rgb], [a])[0][0] for a in (0.3, -0.2)]
    src = image("u8", 0, W, H)                                           # nothing but 0xA5 yet
    dst = [image("u8", 0, W, H), image("u8", 0, W, H)]
    try:
        with v.Stream(0) as st, v.Rotator(W, H, max_batch=1) as rot:
            host = np.full(src.total, D.FILL, dtype=np.uint8)
            host[src.mask] = rgb.reshape(-1)
            src.buf.upload(host, stream=st)
            rot.rotate(src.image, dst[0].image, 0.3, st)
            rot.rotate(src.image, dst[1].image, -0.2, st)
            got = [d.read(st) for d in dst]
        for (raw, clean), w in zip(got, want):
            assert clean and (raw == w).all()
        assert not (want[0] == want[1]).all()
    finally:
        for im in [src] + dst:
            im.close()


def test_validation_before_any_launch():
    """each refused call returns FFTUP_E_INVALID_ARG, names the rule, and leaves the output untouched (all 0xA5)"""
    import vkresample_amd as v
    from vkresample_amd import _lib
    lib = _lib.load()
    W, H = 64, 32
    src = image("u8", 0, W, H, K.frames_u8(W, H)[0])
    dst = image("u8", 0, W, H)
    hostmem = np.zeros(3 * W * H, dtype=np.uint8)
    try:
        with v.Rotator(W, H) as rot:
            a = (_lib.DeviceImageDesc * 1)(src.image.desc())
            b = (_lib.DeviceImageDesc * 1)(dst.image.desc())
            ok = (_lib.Rotation * 1)(_lib.Rotation(0.1, 31.5, 15.5))
            host_in = (_lib.DeviceImageDesc * 1)(_lib.DeviceImageDesc(hostmem.ctypes.data, D.RGB8, 3 * W, 0))
            short = (_lib.DeviceImageDesc * 1)(_lib.DeviceImageDesc(dst.image.ptr, D.RGB8, 3 * W - 1, 0))
            calls = [
                ((a, b, None, 1), "rotations is null"),
                ((a, b, ok, 0), "n_frames must be > 0"),
                ((a, b, (_lib.Rotation * 1)(_lib.Rotation(float("nan"), 31.5, 15.5)), 1), "rotations[0].angle is not finite"),
                ((a, b, (_lib.Rotation * 1)(_lib.Rotation(0.1, float("inf"), 15.5)), 1), "rotations[0]: the centre is not finite"),
                ((a, b, (_lib.Rotation * 1)(_lib.Rotation(1.6, 31.5, 15.5)), 1), "rotations[0].angle is beyond pi / 2"),
                ((host_in, b, ok, 1), "in[0].data is not device memory"),
                ((a, short, ok, 1), "out[0].row_stride_bytes %d is below one row" % (3 * W - 1)),
                ((None, b, ok, 1), "null image array"),
            ]
            for args, piece in calls:
                code = lib.fftup_rotate_frames(rot._h, args[0], args[1], args[2], args[3], None)
                text = lib.fftup_last_error().decode()
                assert code == 1 and piece in text, (code, text, piece)
            raw, clean = dst.read()
            assert clean and (raw == D.FILL).all()
            assert rot.info["num_kernels"] == 3 and rot.info["kernel_names"] == ["rotate_shear_x_in", "rotate_shear_y", "rotate_shear_x_out"]
            assert rot.info["max_batch"] == 4 and rot.info["device_bytes"] >= 2 * 4 * 12 * W * H
    finally:
        src.close()
        dst.close()


def _cli(args, **kw):
    return subprocess.run([P.CLI] + args, capture_output=True, text=True, timeout=120, **kw)


def test_cli_rotate(tmp_path):
    """-rotate 0 writes the bytes of a run without the flag; -rotate 10 on a small PNG equals the Python path: Rotator, then the
    plan through execute_device"""
    import vkresample_amd as v
    W, H = 96, 80
    rgb = P.frame(W, H, 5)
    src = str(tmp_path / "in.png")
    P.png_write(src, rgb)
    outs = {}
    for name, extra in (("plain", []), ("zero", ["-rotate", "0"]), ("ten", ["-rotate", "10"]), ("off", ["-rotate", "10", "-rotatecentre", "30,50.5"])):
        o = str(tmp_path / (name + ".png"))
        p = _cli(["-i", src, "-o", o, "-u", "2"] + extra)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        outs[name] = open(o, "rb").read()
    assert outs["zero"] == outs["plain"]
    assert outs["ten"] != outs["plain"] and outs["off"] != outs["ten"]
    for name, rotn in (("ten", np.deg2rad(10.0)), ("off", (np.deg2rad(10.0), 30.0, 50.5))):
        a = image("u8", 0, W, H, rgb)
        b = image("u8", 0, W, H)
        with v.Upscaler(W, H, 2.0, 0, 0.2, 0) as up:
            c = D.Image(D.RGB8, up.out_width, up.out_height, 4)
            try:
                with v.Rotator(W, H) as rot:
                    rot.rotate(a.image, b.image, rotn)
                    up.execute_device(b.image, c.image)
                    want = c.read()[0].reshape(up.out_height, up.out_width, 3)
            finally:
                for im in (a, b, c):
                    im.close()
        got = P.png_pixels(outs[name], up.out_width, up.out_height)
        assert (np.asarray(got).reshape(want.shape) == want).all(), name
