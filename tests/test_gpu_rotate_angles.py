"""GPU: fftup_rotate_frames_angles (Rotator.frames_angles) -- the rotator with its angles read in device memory -- and the chain it
closes: roll estimate -> rotation by -angle -> shift estimate, on one stream with nothing read by the host in between.

The yardstick is tests/rotate_oracle.py at theta_i = rotations[i].angle + gain * (double)angle_i, a device angle that is not finite
counting as 0 and theta_i clamped to [-pi/2, pi/2]; the bars are the rotator's own, FP32_ABS and FP32_REL_L2 of
tests/rotate_cases.py (four times the complex64 oracle's difference to the complex128 oracle, kept honest by
tests/test_rotate_bars.py) -- imported, not copied.  The host path computes tan and sin with the host's libm and the device path
with the device's: the two may differ in the last place of a double, which is why the result is held to the oracle and not to
fftup_rotate_frames byte for byte.

Measured on an MI355X: float planes within 5.4e-7 and 2.1e-7 relative L2 of the oracle at theta_i on all three sizes and both gains
(bars 2.56e-6 and 8.4e-7); gain = 0 gave the host path's bytes exactly; the chain's shift within 0.0096 pixels of R(-theta) t (bar
0.064, of which the lever arm is 0.014)."""
import numpy as np
import pytest

import align_oracle as AO
import devimage as D
import paritylib as P
import roll_cases as RC
import roll_oracle as RL
import rotate_cases as K
import rotate_oracle as R

pytestmark = pytest.mark.gpu

SIZES = [(64, 32), (45, 21), (96, 80)]
DEVICE_ANGLES = [0.0, 0.02, -0.3, float("nan"), 3.0]
HOST_ANGLE = 0.1


def theta_of(host, gain, dev):
    """what the device forms: double arithmetic on the fp32 angle widened to double"""
    m = np.float32(dev)
    t = float(host) + float(gain) * (float(m) if np.isfinite(m) else 0.0)
    return min(max(t, -np.pi / 2), np.pi / 2)


class _Angles:
    """fftup_roll_angle records in device memory: the given angles, peak = NaN (never read), between guard bands"""

    def __init__(self, angles):
        import vkresample_amd as v
        rec = np.zeros((len(angles), 4), np.float32)
        rec[:, 0] = angles
        rec[:, 1:3] = np.nan
        host = np.full(2 * D.GUARD + rec.nbytes, D.FILL, np.uint8)
        host[D.GUARD:D.GUARD + rec.nbytes] = rec.reshape(-1).view(np.uint8)
        self.host = host
        self.buf = v.DeviceBuffer(host.size)
        self.buf.upload(host)
        self.ptr = self.buf.ptr + D.GUARD

    def unchanged(self):
        return bool((self.buf.download() == self.host).all())

    def close(self):
        self.buf.close()


def _planes(W, H, frame=None, padded=False):
    return D.Image(D.PLANAR, W, H, 4, padded, D.GUARD, frame)


def _values(raw, W, H):
    return raw.view(np.float32).reshape(3, H, W).astype(np.float64)


@pytest.mark.parametrize("gain", [1.0, -1.0])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_parity_with_the_oracle_at_the_device_angles(size, gain):
    """five frames, float planes, on a rotator with max_batch = 3 (chunks of 3 and 2: the coefficient buffer is indexed within the
    chunk, the device angles across it), host angle 0.1 about a centre off the frame's: device angles 0, 0.02, -0.3, NaN (counts as
    0) and 3.0 (0.1 + 3.0 clamps to pi/2, 0.1 - 3.0 to -pi/2).  Output within FP32_ABS and FP32_REL_L2 of the oracle at theta_i;
    padding and guards untouched; the angle records unchanged."""
    import vkresample_amd as v
    W, H = size
    centre = (W / 3.0, 2.0 * H / 3.0 + 0.5)
    frames = [R.planes_of(f).astype(np.float32) for f in K.frames_u8(W, H)[:5]]
    src = [_planes(W, H, f, padded=(i % 2 == 1)) for i, f in enumerate(frames)]
    dst = [_planes(W, H, None, padded=(i % 2 == 0)) for i in range(5)]
    ang = _Angles(DEVICE_ANGLES)
    try:
        with v.Rotator(W, H, 0, 0, 3) as rot:
            rot.frames_angles([s.image for s in src], [d.image for d in dst], [(HOST_ANGLE,) + centre] * 5, ang.ptr, gain)
            out = [d.read() for d in dst]
            assert ang.unchanged()
    finally:
        for im in src + dst:
            im.close()
        ang.close()
    thetas = [theta_of(HOST_ANGLE, gain, a) for a in DEVICE_ANGLES]
    assert thetas[3] == HOST_ANGLE and abs(thetas[4]) == np.pi / 2
    for i, ((raw, clean), f, t) in enumerate(zip(out, frames, thetas)):
        want = R.rotate(f.astype(np.float64), t, centre)
        got = _values(raw, W, H)
        P.measured("rotate angles %dx%d gain %+g frame %d theta %+.4f" % (W, H, gain, i, t), max_abs=np.abs(got - want).max(), rel_l2=P.rel_l2(got, want))
        assert clean
        assert np.abs(got - want).max() <= K.FP32_ABS
        assert P.rel_l2(got, want) <= K.FP32_REL_L2


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_gain_zero_is_the_host_path(size):
    """gain = 0: theta_i is the host angle whatever the device holds; the output equals fftup_rotate_frames' within the rotator's
    bars (not byte for byte: tan and sin of the device against the host's)"""
    import vkresample_amd as v
    W, H = size
    frames = [R.planes_of(f).astype(np.float32) for f in K.frames_u8(W, H)[:5]]
    rots = [0.3, -0.2, 0.0, 0.7, -1.1]
    src = [_planes(W, H, f) for f in frames]
    dst = [_planes(W, H) for _ in range(10)]
    ang = _Angles(DEVICE_ANGLES)
    try:
        with v.Rotator(W, H, 0, 0, 2) as rot:
            rot.rotate([s.image for s in src], [d.image for d in dst[:5]], rots)
            rot.frames_angles([s.image for s in src], [d.image for d in dst[5:]], rots, ang.ptr, 0.0)
            out = [_values(d.read()[0], W, H) for d in dst]
    finally:
        for im in src + dst:
            im.close()
        ang.close()
    for i in range(5):
        P.measured("rotate angles %dx%d gain 0 frame %d" % (W, H, i), max_abs=np.abs(out[i] - out[5 + i]).max(), rel_l2=P.rel_l2(out[5 + i], out[i]),
                   identical=float((out[i] == out[5 + i]).all()))
        assert np.abs(out[i] - out[5 + i]).max() <= K.FP32_ABS and P.rel_l2(out[5 + i], out[i]) <= K.FP32_REL_L2


def test_refusals_enqueue_nothing():
    """each refused call returns FFTUP_E_INVALID_ARG, names the rule, and leaves the output untouched (all 0xA5)"""
    import vkresample_amd as v
    from vkresample_amd import _lib
    lib = _lib.load()
    W, H = 64, 32
    src = D.Image(D.RGB8, W, H, 4, False, D.GUARD, K.frames_u8(W, H)[0])
    dst = D.Image(D.RGB8, W, H, 4)
    ang = _Angles([0.1])
    hostmem = np.zeros(3 * W * H, dtype=np.uint8)
    try:
        with v.Rotator(W, H) as rot:
            a = (_lib.DeviceImageDesc * 1)(src.image.desc())
            b = (_lib.DeviceImageDesc * 1)(dst.image.desc())
            ok = (_lib.Rotation * 1)(_lib.Rotation(0.1, 31.5, 15.5))
            host_in = (_lib.DeviceImageDesc * 1)(_lib.DeviceImageDesc(hostmem.ctypes.data, D.RGB8, 3 * W, 0))
            short = (_lib.DeviceImageDesc * 1)(_lib.DeviceImageDesc(dst.image.ptr, D.RGB8, 3 * W - 1, 0))
            calls = [
                ((a, b, ok, None, -1.0, 1), "angles_device is null"),
                ((a, b, ok, ang.ptr + 2, -1.0, 1), "angles_device is not a multiple of 4 bytes"),
                ((a, b, ok, hostmem.ctypes.data, -1.0, 1), "angles_device is not device memory"),
                ((a, b, ok, ang.ptr, float("nan"), 1), "gain is not finite"),
                ((a, b, ok, ang.ptr, float("-inf"), 1), "gain is not finite"),
                ((a, b, None, ang.ptr, -1.0, 1), "rotations is null"),
                ((a, b, ok, ang.ptr, -1.0, 0), "n_frames must be > 0"),
                ((a, b, (_lib.Rotation * 1)(_lib.Rotation(float("nan"), 31.5, 15.5)), ang.ptr, -1.0, 1), "rotations[0].angle is not finite"),
                ((a, b, (_lib.Rotation * 1)(_lib.Rotation(0.1, float("inf"), 15.5)), ang.ptr, -1.0, 1), "rotations[0]: the centre is not finite"),
                ((a, b, (_lib.Rotation * 1)(_lib.Rotation(1.6, 31.5, 15.5)), ang.ptr, -1.0, 1), "rotations[0].angle is beyond pi / 2"),
                ((host_in, b, ok, ang.ptr, -1.0, 1), "in[0].data is not device memory"),
                ((a, short, ok, ang.ptr, -1.0, 1), "out[0].row_stride_bytes %d is below one row" % (3 * W - 1)),
                ((None, b, ok, ang.ptr, -1.0, 1), "null image array"),
            ]
            for args, piece in calls:
                code = lib.fftup_rotate_frames_angles(rot._h, args[0], args[1], args[2], args[3], args[4], args[5], None)
                text = lib.fftup_last_error().decode()
                assert code == 1 and piece in text, (code, text, piece)
            raw, clean = dst.read()
            assert clean and (raw == D.FILL).all()
            # ... and the rotator is none the worse for it: the accepted call still works.  The host angle is the device's fp32 0.1
            # widened to double, so theta = 0 exactly and the 8-bit frame comes back byte for byte
            rot.frames_angles(src.image, dst.image, (float(np.float32(0.1)), 31.5, 15.5), ang.ptr, -1.0)
            raw, clean = dst.read()
            assert clean and (raw.reshape(H, W, 3) == K.frames_u8(W, H)[0]).all()
    finally:
        src.close()
        dst.close()
        ang.close()


def test_chain_roll_rotate_align_on_one_stream():
    """160 x 160, four frames of the roll scene (turned by 0, 0.004, -0.02, 0.05 and moved): fftup_roll_angles, then
    fftup_rotate_frames_angles with gain = -1 about the frame centre, then fftup_align_shifts of the de-rotated frames against the
    reference -- all enqueued on ONE stream behind the uploads, with a single wait at the end (the read-back): had any step needed a
    host copy, it would have read what was not yet written.
    A frame shows scene(c + R(-a)(p - c - t)); turned back by the estimate a' it shows scene(c + R(a' - a)(p - c) - R(-a) t): the
    shift to recover is R(-a) t, and what is left of the roll, e = a' - a, moves a pixel at distance r from the centre by e r.
    Bar: the aligner's own 0.05 window pixels against ground truth at this window (tests/test_align_oracle.py, BAR) plus the lever
    arm e r, with e the ORACLE's largest roll error over these four pairs plus the roll parity bar, and r half the diagonal of the
    aligner's window -- computed below, nothing guessed."""
    import vkresample_amd as v
    case = RL.GPU_CASES[1]
    W, H, window, d = case
    ref, moved, true = RC.scene(case)
    moved, true = moved[:4], true[:4]
    ga = AO.geometry(W, H)
    assert (ga["nx"], ga["ny"], ga["d"]) == (128, 128, 1)
    roll_error = max(abs(o["angle"] - a) for o, a in zip(RC.oracle(case, "rgb8")[:4], true)) + RC.bars()["angle"]
    lever = roll_error * 0.5 * np.hypot(ga["nx"] * ga["d"], ga["ny"] * ga["d"])
    bar = 0.05 * ga["d"] + lever
    want = []
    for a, (tx, ty) in zip(true, RL.MOVES):
        c, s = np.cos(a), np.sin(a)
        want.append((c * tx * d + s * ty * d, -s * tx * d + c * ty * d))
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    src = [D.Image(D.RGB8, W, H, 4) for _ in range(5)]                  # nothing but 0xA5 yet
    mid = [D.Image(D.RGB8, W, H, 4) for _ in range(4)]
    ang = v.DeviceBuffer(4 * 16)
    shf = v.DeviceBuffer(4 * 16)
    try:
        with v.Stream(0) as st, v.Roller(W, H, window=window, decimate=d) as ro, v.Rotator(W, H) as rot, v.Aligner(W, H) as al:
            for im, f in zip(src, [ref] + list(moved)):
                host = np.full(im.total, D.FILL, dtype=np.uint8)
                host[im.mask] = f.reshape(-1)
                im.buf.upload(host, stream=st)
            ro.angles_device(src[0].image, [s.image for s in src[1:]], ang.ptr, st)
            rot.frames_angles([s.image for s in src[1:]], [m.image for m in mid], [(0.0, cx, cy)] * 4, ang.ptr, -1.0, st)
            al.shifts_device(src[0].image, [m.image for m in mid], shf.ptr, st)
            shifts = shf.download(stream=st).view(np.float32).reshape(4, 4).copy()     # the one wait
            angles = ang.download(stream=st).view(np.float32).reshape(4, 4).copy()
    finally:
        for im in src + mid:
            im.close()
        ang.close()
        shf.close()
    for k in range(4):
        err = float(np.hypot(shifts[k][0] - want[k][0], shifts[k][1] - want[k][1]))
        P.measured("chain 160x160 frame %d" % k, true_angle=true[k], angle=angles[k][0], shift_x=shifts[k][0], shift_y=shifts[k][1],
                   want_x=want[k][0], want_y=want[k][1], error=err, bar=bar, lever=lever, peak=shifts[k][2])
    for k in range(4):
        assert abs(angles[k][0] - true[k]) <= RL.ACCURACY_BAR[(W, H)]
        assert abs(shifts[k][0] - want[k][0]) <= bar and abs(shifts[k][1] - want[k][1]) <= bar, (k, shifts[k], want[k])
        assert shifts[k][2] >= 0.5
