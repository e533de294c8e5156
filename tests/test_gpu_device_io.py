"""GPU: fftup_execute_device (Upscaler.execute_device) -- a plan run on caller-owned device memory.

The yardstick throughout is the SAME plan's host path, upload_* -> execute(1) -> download_*, compared byte for byte: the frame
kernels are the same ones, only the pointers and strides they are launched with differ, and the staging kernels (gather, scatter,
strided pack) move or convert values exactly as the host path's copies and conversion launches do.  No tolerance is involved.

Every output image sits in a buffer with 256-byte guard bands in front and behind, pre-filled with 0xA5 like all row and plane
padding (tests/devimage.py): after the run the pixels equal the host path's and every other byte is still 0xA5 (write containment).

Run directly (`python tests/test_gpu_device_io.py batch`) the file performs the batch check in a process of its own: the test that
pins FFTUP_STREAMS=1 starts it that way, because the variable is read at plan creation of a fresh process."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from devimage import DTYPE, ESZ, FILL, GUARD, PLANAR, RGB8, Image, device_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _make(key):
    import vkresample_amd as v
    U = v.Upscaler
    return {
        "default": lambda: U(64, 32, 2.0, 0),
        "default_p2": lambda: U(64, 32, 2.0, 2),
        "generic": lambda: U(240, 126, 2.0, 0, flags=v.FLAG_GENERIC_KERNELS),
        "generic_p2": lambda: U(240, 126, 2.0, 2, flags=v.FLAG_GENERIC_KERNELS),
        "u8store_p2": lambda: U(512, 256, 2.0, 2, flags=v.FLAG_FUSE_U8_LOAD | v.FLAG_FUSE_U8_STORE),
        "exact_centre": lambda: U.to_size(50, 32, 32, 50, align=v.ALIGN_CENTRE),
        "odd": lambda: U(45, 21, 2.0, 0, flags=v.FLAG_ODD_SIZE),
        "odd_p2": lambda: U(45, 21, 2.0, 2, flags=v.FLAG_ODD_SIZE),
        "bluestein": lambda: U(46, 22, 2.0, 0, flags=v.FLAG_ANY_SIZE),
        "dct": lambda: U(64, 32, 2.0, 0, flags=v.FLAG_DCT),
        "down": lambda: U(128, 64, 0.5, 0, flags=v.FLAG_DOWNSCALE),
        "double": lambda: U(20, 12, 2.0, 1),
    }[key]()


ITEM1 = ["default", "generic", "u8store_p2", "exact_centre", "odd", "bluestein", "dct", "down", "double"]

_plans, _host_cache = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_plans():
    yield
    for up in _plans.values():
        up.close()
    _plans.clear()
    _host_cache.clear()
    _fresh_cache.clear()


def _plan(key):
    if key not in _plans:
        _plans[key] = _make(key)
    return _plans[key]


def _plan_frame(up, fmt, seed):
    """a W x H input frame: uint8 [H][W][3] or planes [3][H][W] of the plan's storage type with values in [0, 1)"""
    from vkresample_amd import synth
    if fmt == RGB8:
        return synth.frame(seed, up.width, up.height, "N")
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    return rng.random((3, up.height, up.width)).astype(DTYPE[up.precision])


def _host_run(up, fmt, frame):
    """the yardstick: {PLANAR: bytes of download_planar (plans with planes), RGB8: bytes of download_rgb8}"""
    if fmt == RGB8:
        up.upload_rgb8(frame)
    else:
        up.upload_planar(frame)
    up.execute(1)
    res = {RGB8: up.download_rgb8().reshape(-1).copy()}
    if not up.u8_store:
        res[PLANAR] = up.download_planar().reshape(-1).view(np.uint8).copy()
    return res


def _host(key, fmt, seed=7):
    """computed once per (plan, input format, frame), shared and left unchanged"""
    k = (key, fmt, seed)
    if k not in _host_cache:
        up = _plan(key)
        _host_cache[k] = _host_run(up, fmt, _plan_frame(up, fmt, seed))
        for a in _host_cache[k].values():
            a.flags.writeable = False
    return _host_cache[k]


# ---------------------------------------------------------------- 1. equality over the plan kinds, dense, guard bands checked
@pytest.mark.parametrize("fmt_out", [RGB8, PLANAR], ids=["out_rgb8", "out_planar"])
@pytest.mark.parametrize("fmt_in", [RGB8, PLANAR], ids=["in_rgb8", "in_planar"])
@pytest.mark.parametrize("key", ITEM1)
def test_equals_host_path(key, fmt_in, fmt_out):
    import vkresample_amd as v
    up = _plan(key)
    want = _host(key, fmt_in)
    frame = _plan_frame(up, fmt_in, 7)
    if key == "u8store_p2":
        assert up.u8_store
    if up.u8_store and fmt_out == PLANAR:
        with pytest.raises(v.FftupError) as e:          # no planes on such a plan: the rule of fftup_download_planar
            device_run(up, fmt_in, frame, fmt_out)
        assert e.value.code == 1 and "FFTUP_FLAG_FUSE_U8_STORE" in str(e.value)
        return
    got, clean = device_run(up, fmt_in, frame, fmt_out)
    assert np.array_equal(got, want[fmt_out])
    assert clean, "bytes outside the image were written"


# ---------------------------------------------------------------- 2. strides and containment
@pytest.mark.parametrize("fmt_out", [RGB8, PLANAR], ids=["out_rgb8", "out_planar"])
@pytest.mark.parametrize("fmt_in", [RGB8, PLANAR], ids=["in_rgb8", "in_planar"])
@pytest.mark.parametrize("key", ["generic", "generic_p2", "odd", "odd_p2"])
def test_padded_rows_and_planes(key, fmt_in, fmt_out):
    up = _plan(key)
    want = _host(key, fmt_in)
    got, clean = device_run(up, fmt_in, _plan_frame(up, fmt_in, 7), fmt_out, in_padded=True, out_padded=True)
    assert np.array_equal(got, want[fmt_out])
    assert clean, "row padding, plane padding or a guard band was written"


def test_padded_rows_of_a_fused_8bit_store():
    """FFTUP_FLAG_FUSE_U8_STORE with padded output rows: lane scratch + strided byte copy"""
    up = _plan("u8store_p2")
    want = _host("u8store_p2", RGB8)
    got, clean = device_run(up, RGB8, _plan_frame(up, RGB8, 7), RGB8, in_padded=True, out_padded=True)
    assert np.array_equal(got, want[RGB8]) and clean


# ---------------------------------------------------------------- 3. misaligned planes
@pytest.mark.parametrize("offset", ["element", "byte"])
@pytest.mark.parametrize("key", ["default", "default_p2", "generic", "generic_p2"])
def test_misaligned_planar_input(key, offset):
    """`data` one element behind a 256-byte boundary: read in place (the first kernels load single elements); one BYTE behind it:
    through the gather kernel into the lane's staging planes.  The same bytes as the aligned run's either way."""
    up = _plan(key)
    frame = _plan_frame(up, PLANAR, 7)
    aligned, clean0 = device_run(up, PLANAR, frame, PLANAR)
    off = ESZ[up.precision] if offset == "element" else 1
    got, clean = device_run(up, PLANAR, frame, PLANAR, in_base=GUARD + off)
    assert np.array_equal(got, aligned) and np.array_equal(got, _host(key, PLANAR)[PLANAR])
    assert clean0 and clean


@pytest.mark.parametrize("offset", ["element", "byte"])
@pytest.mark.parametrize("key", ["default", "default_p2", "u8store_p2"])
def test_misaligned_output(key, offset):
    """dense planes that are not 16-byte aligned go through the lane scratch and the scatter kernel (the last kernels store up to 16
    bytes at once); the fused 8-bit store writes single bytes and takes any address"""
    up = _plan(key)
    fmt = RGB8 if up.u8_store else PLANAR
    off = ESZ[up.precision] if offset == "element" else 1
    got, clean = device_run(up, RGB8, _plan_frame(up, RGB8, 7), fmt, out_base=GUARD + off)
    assert np.array_equal(got, _host(key, RGB8)[fmt]) and clean


# ---------------------------------------------------------------- 4. batch
def _batch_check():
    """five distinct frames through one call on a ring = 1 plan: each output equals that frame's own host-path result"""
    import vkresample_amd as v
    with v.Upscaler(64, 32, 2.0, 0, ring=1) as up:
        frames = [_plan_frame(up, RGB8, 20 + i) for i in range(5)]
        want = [_host_run(up, RGB8, f)[PLANAR] for f in frames]
        assert len({w.tobytes() for w in want}) == 5
        src = [Image(RGB8, 64, 32, 4, frame=f) for f in frames]
        dst = [Image(PLANAR, 128, 64, 4) for _ in frames]
        try:
            up.execute_device([s.image for s in src], [d.image for d in dst])
            for d, w in zip(dst, want):
                got, clean = d.read()
                assert np.array_equal(got, w) and clean
            # the tap belongs to the call's last frame
            tap = up.download_presharpen()
            _host_run(up, RGB8, frames[4])
            assert np.array_equal(tap, up.download_presharpen())
        finally:
            for i in src + dst:
                i.close()


def test_batch_of_five_frames():
    _batch_check()


def test_batch_of_five_frames_on_one_stream():
    env = dict(os.environ, FFTUP_STREAMS="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "batch"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"batch ok" in r.stdout, r.stdout.decode(errors="replace")[-2000:]


# ---------------------------------------------------------------- 5. ordering without host synchronisation
@pytest.mark.parametrize("own_stream", [True, False], ids=["stream", "default_stream"])
def test_two_plans_chained_on_one_stream(own_stream):
    """A: 64x32 -> 128x64, B: 128x64 -> 64x32 (downscale), B reading what A writes, with nothing but the stream between them"""
    import vkresample_amd as v
    A, B = _plan("default"), _plan("down")
    x = _plan_frame(A, PLANAR, 31)
    A.upload_planar(x)
    A.execute(1)
    B.upload_planar(A.download_planar())
    B.execute(1)
    want = B.download_planar().reshape(-1).view(np.uint8)
    s = v.Stream() if own_stream else None
    src = Image(PLANAR, 64, 32, 4)
    mid = Image(PLANAR, 128, 64, 4)
    dst = Image(PLANAR, 64, 32, 4)
    try:
        host = np.full(src.total, FILL, dtype=np.uint8)
        host[src.mask] = x.reshape(-1).view(np.uint8)
        src.buf.upload(host, stream=s)
        A.execute_device(src.image, mid.image, s)
        B.execute_device(mid.image, dst.image, s)
        got, clean = dst.read(s)
        assert np.array_equal(got, want) and clean
    finally:
        for i in (src, mid, dst):
            i.close()
        if s is not None:
            s.close()


# ---------------------------------------------------------------- 6. validation
def test_invalid_descriptors_are_refused_before_any_launch():
    import vkresample_amd as v
    up = _plan("default")
    frame = _plan_frame(up, RGB8, 7)
    src = Image(RGB8, 64, 32, 4, frame=frame)
    srcp = Image(PLANAR, 64, 32, 4, frame=_plan_frame(up, PLANAR, 7))
    dst = Image(PLANAR, 128, 64, 4)
    host_rgb = np.ascontiguousarray(frame)
    good_in, good_out = src.image, dst.image
    cases = [
        (v.DeviceImage(host_rgb.ctypes.data, RGB8, 3 * 64), good_out, "device"),
        (v.DeviceImage(src.image.ptr, RGB8, 3 * 64 - 1), good_out, "row_stride"),
        (v.DeviceImage(srcp.image.ptr, PLANAR, 64 * 4 + 2, 32 * (64 * 4 + 2) + 2), good_out, "multiple"),
        (v.DeviceImage(src.image.ptr, 7, 3 * 64), good_out, "format"),
        (good_in, v.DeviceImage(dst.image.ptr, 7, 128 * 4, 128 * 64 * 4), "format"),
        (good_in, v.DeviceImage(dst.image.ptr, PLANAR, 128 * 4 - 4, 128 * 64 * 4), "row_stride"),
        (good_in, v.DeviceImage(dst.image.ptr, PLANAR, 128 * 4, 128 * 64 * 4 - 4), "plane_stride"),
        (good_in, v.DeviceImage(None, PLANAR, 128 * 4, 128 * 64 * 4), "null"),
    ]
    try:
        for a, b, word in cases:
            with pytest.raises(v.FftupError) as e:
                up.execute_device(a, b)
            assert e.value.code == 1 and word in str(e.value), str(e.value)
            got = dst.buf.download()
            assert (got == FILL).all(), word
        with pytest.raises(v.FftupError) as e:
            up.execute_device([], [])
        assert e.value.code == 1 and "n_frames" in str(e.value)
        assert (dst.buf.download() == FILL).all()
    finally:
        for i in (src, srcp, dst):
            i.close()


# ---------------------------------------------------------------- 7. the ring slots are neither read nor written
def test_slots_untouched():
    up = _plan("default")
    f0, f1 = _plan_frame(up, RGB8, 40), _plan_frame(up, RGB8, 41)
    up.upload_rgb8(f0)
    up.execute(1)
    planes, word_sum = up.download_planar().copy(), up.output_checksum(0)
    other = _host("default", RGB8, 41)[PLANAR]
    up.upload_rgb8(f0)
    up.execute(1)
    assert np.array_equal(up.download_planar(), planes)
    got, clean = device_run(up, RGB8, f1, PLANAR)
    assert np.array_equal(got, other) and clean and not np.array_equal(got, planes.reshape(-1).view(np.uint8))
    assert np.array_equal(up.download_planar(0), planes) and up.output_checksum(0) == word_sum
    up.execute(1)                                          # ... and the input slot still holds f0
    assert np.array_equal(up.download_planar(0), planes) and up.output_checksum(0) == word_sum


# ---------------------------------------------------------------- 8. what the last frame left behind: its lane, its tap
# 512x256 -> 1024x512 is the smallest plan with ahead-of-time fused kernels; the default three streams.  The yardstick is a fresh
# ring = 1 plan: upload -> execute(1) -> downloads, byte for byte.
FS_W, FS_H = 512, 256
SEED_A, SEED_B, SEED_C = 61, 62, 63
_fresh_cache = {}


def _fs_plan(precision, flags=0, ring=2):
    import vkresample_amd as v
    return v.Upscaler(FS_W, FS_H, 2.0, precision, flags=flags, ring=ring)


def _fs_frame(seed):
    from vkresample_amd import synth
    return synth.frame(seed, FS_W, FS_H, "N")


def _fresh(precision, flags, seed, planar=False):
    """{"out", "tap", "rgb8"} of one frame on a fresh ring = 1 plan after execute(1); computed once, shared and left unchanged.
    The fresh plan carries FFTUP_FLAG_OVERLAP_ITERATIONS: the strip length of the fused C2R+sharpen kernel is a property of the
    plan, chosen by whether its frames overlap (strip_length, plan_rules.cpp), and fp32 outputs depend on the cuts in their last
    bits (test_fused_output_independent_of_strip_length) -- without the flag a ring = 1 plan cuts a frame differently from the
    ring = 2 plan under test and their fp32 outputs differ (taps, binary16 and unfused outputs do not).  One iteration runs on
    lane 0 with or without it."""
    import vkresample_amd as v
    k = (precision, flags, seed, planar)
    if k not in _fresh_cache:
        with _fs_plan(precision, flags | v.FLAG_OVERLAP_ITERATIONS, ring=1) as up:
            if planar:
                up.upload_planar(_plan_frame(up, PLANAR, seed))
            else:
                up.upload_rgb8(_fs_frame(seed))
            up.execute(1)
            res = {"out": up.download_planar(), "tap": up.download_presharpen(), "rgb8": up.download_rgb8()}
        for a in res.values():
            a.flags.writeable = False
        _fresh_cache[k] = res
    return _fresh_cache[k]


def _ring_run_ab(up):
    """A in slot 0, B in slot 1, two frames: with more than one stream the run ends on lane 1"""
    up.upload_rgb8(_fs_frame(SEED_A), slot=0)
    up.upload_rgb8(_fs_frame(SEED_B), slot=1)
    up.execute_ring(2)


def _unfused():
    import vkresample_amd as v
    return v.FLAG_UNFUSED_SHARPEN


FS_CASES = [(0, False), (2, False), (0, True), (2, True)]
FS_IDS = ["p0", "p2", "p0_unfused", "p2_unfused"]


@pytest.mark.parametrize("precision,unfused", FS_CASES, ids=FS_IDS)
def test_tap_after_a_ring_run_that_ends_on_lane_1(precision, unfused):
    """fused plans: the tap is rebuilt from lane 1's spectra; unfused ones: it is lane 1's own pre-sharpen image"""
    flags = _unfused() if unfused else 0
    a, b = _fresh(precision, flags, SEED_A), _fresh(precision, flags, SEED_B)
    assert not np.array_equal(a["tap"], b["tap"])
    with _fs_plan(precision, flags) as up:
        _ring_run_ab(up)
        assert np.array_equal(up.download_planar(0), a["out"])
        assert np.array_equal(up.download_planar(1), b["out"])
        assert np.array_equal(up.download_presharpen(), b["tap"])


@pytest.mark.parametrize("precision", [0, 2], ids=["p0", "p2"])
def test_tap_after_the_queue_ends_on_lane_1(precision):
    a, b = _fresh(precision, 0, SEED_A), _fresh(precision, 0, SEED_B)
    with _fs_plan(precision) as up:
        ins = np.stack([_fs_frame(SEED_A), _fs_frame(SEED_B)])
        outs = np.zeros((2, 2 * FS_H, 2 * FS_W, 3), np.uint8)
        for k in range(2):
            up.submit_rgb8(ins[k], outs[k])
        up.drain()
        assert np.array_equal(outs[0], a["rgb8"]) and np.array_equal(outs[1], b["rgb8"])
        assert np.array_equal(up.download_presharpen(), b["tap"])


@pytest.mark.parametrize("precision,unfused", FS_CASES, ids=FS_IDS)
def test_tap_follows_profile_kernels(precision, unfused):
    """profile_kernels(1) runs slot 0 (frame A) on lane 0 after a ring run that ended on lane 1 with frame B: the tap belongs to
    the frame that ran last, A.  (Before the frame context, fftup_profile_kernels left the tap's lane as the ring run had set it,
    and the tap returned B's: assertion failure on every one of the four cases.)"""
    flags = _unfused() if unfused else 0
    a, b = _fresh(precision, flags, SEED_A), _fresh(precision, flags, SEED_B)
    with _fs_plan(precision, flags) as up:
        _ring_run_ab(up)
        assert np.array_equal(up.download_presharpen(), b["tap"])
        up.profile_kernels(1)
        assert np.array_equal(up.download_presharpen(), a["tap"])


@pytest.mark.parametrize("precision", [0, 2], ids=["p0", "p2"])
def test_ring_run_device_frame_ring_run_leave_nothing_behind(precision):
    """ring run, a device frame C (planes one byte off alignment: staged; padded 8-bit output: lane scratch + strided pack), the
    same ring run again: the second run's slots and checksums equal the first's, and C equals C through the host path"""
    c = _fresh(precision, 0, SEED_C, planar=True)
    with _fs_plan(precision) as up:
        _ring_run_ab(up)
        first = [(up.download_planar(s), up.output_checksum(s)) for s in range(2)]
        got, clean = device_run(up, PLANAR, _plan_frame(up, PLANAR, SEED_C), RGB8, out_padded=True, in_base=GUARD + 1)
        assert np.array_equal(got, c["rgb8"].reshape(-1)) and clean
        up.execute_ring(2)
        for s in range(2):
            assert np.array_equal(up.download_planar(s), first[s][0]) and up.output_checksum(s) == first[s][1]
        assert np.array_equal(first[0][0], _fresh(precision, 0, SEED_A)["out"])
        assert np.array_equal(first[1][0], _fresh(precision, 0, SEED_B)["out"])


if __name__ == "__main__":
    if sys.argv[1:] == ["batch"]:
        _batch_check()
        print("batch ok")
