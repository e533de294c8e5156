"""GPU: fftup_roll_angles (Roller) -- roll estimates of frame pairs in device memory.

The yardstick is tests/roll_oracle.py, the estimate restated in fp64 numpy (itself held to analytically turned scenes by
tests/test_roll_oracle.py), on 8-bit scenes (float and half planes are conversions of the 8-bit frames): computed once per case and
input format (tests/roll_cases.py), shared and left unchanged.

Bars.  angle, peak, peak_coarse: four times the largest difference between the oracle in complex64 and the oracle in complex128
over these cases and formats, computed by roll_cases.bars() when the module loads -- no figure is typed in
(tests/test_roll_bars.py prints them: about 9.6e-7 rad, 2.2e-7 and 3.5e-7).  The coarse cell p is not part of a fftup_roll_angle, but
peak_coarse is the correlation's value AT that cell: where the oracle's best and second-best coarse values differ by 1e-3 of the peak
or more, a library that picked another cell would report a peak_coarse at least that far off -- thousands of bars -- so peak_coarse
within its bar is the same coarse cell.  Where the oracle's gap is smaller the argmax is a coin toss in fp32 (the peak of the
512 x 256 window is broad, a scene can leave two cells that close) and the neighbouring cell is accepted: peak_coarse then has to
match the oracle's value of the best cell or of one of the two beside it.  With the scenes of roll_oracle.CASE_SEED no pair needs
that (the smallest gap is 1.5e-2 of the peak); tests/test_roll_bars.py asserts it, so the branch is not what passes the test.

Measured on an MI355X, all four cases and three formats (pytest -s prints every figure): angle within 2.4e-7 rad (80 x 48; 7.5e-8 to
1.5e-7 elsewhere), peak within 6.0e-8, peak_coarse within 1.2e-7; the oracle's cell everywhere; against the TRUE angles 0.16 mrad at
160 x 160, 1.0 mrad at 320 x 192 with d = 2, 0.10 mrad at 600 x 300."""
import numpy as np
import pytest

import roll_cases as K
import roll_oracle as R
from devimage import FILL, GUARD, PLANAR, RGB8, Image
from paritylib import measured

pytestmark = pytest.mark.gpu

ESZ = {"rgb8": 1, "planar_f32": 4, "planar_f16": 2}


def _images(case, fmt, frames, padded=False, base=GUARD):
    W, H = case[0], case[1]
    return [Image(RGB8 if fmt == "rgb8" else PLANAR, W, H, ESZ[fmt], padded, base, K.FORMATS[fmt][1](f)) for f in frames]


def _roller(case, fmt, **kw):
    import vkresample_amd as v
    W, H, window, d = case
    return v.Roller(W, H, K.FORMATS[fmt][0], window=window, decimate=d, **kw)


def _close(images):
    for im in images:
        im.close()


class _Result:
    """n fftup_roll_angle in device memory between two guard bands of 0xA5"""

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

    def close(self):
        self.buf.close()


# ---------------------------------------------------------------- 1. parity with the oracle
@pytest.mark.parametrize("fmt", list(K.FORMATS))
@pytest.mark.parametrize("case", R.GPU_CASES, ids=K.CASE_IDS)
def test_parity_with_the_oracle(case, fmt):
    """seven pairs in one call with max_batch = 3: chunks of 3, 3 and 1, the buffers reused in stream order.  angle, peak and
    peak_coarse within roll_cases.bars() of the fp64 oracle -- for peak_coarse that is the same coarse cell where the oracle's gap is
    at least 1e-3 of its peak; below that the value of a neighbouring cell is accepted too; reserved is 0."""
    bars = K.bars()
    ref, moved, true = K.scene(case)
    oracle = K.oracle(case, fmt)
    ims = _images(case, fmt, [ref] + list(moved))
    try:
        with _roller(case, fmt, max_batch=3) as ro:
            g = R.geometry(case[0], case[1], case[2], case[3])
            assert (ro.info["window_w"], ro.info["window_h"], ro.info["decimate"], ro.info["angles"], ro.info["rho_min"], ro.info["rho_max"],
                    ro.info["m_band"], ro.info["K"], ro.info["upsample"]) == (g["nx"], g["ny"], g["d"], g["angles"], g["rho_min"], g["rho_max"], g["mb"], g["K"], 32)
            assert ro.info["kernel_names"] == ["roll_rows", "roll_cols", "roll_polar", "roll_peak"] and ro.info["max_batch"] == 3
            got = ro.angles(ims[0].image, [im.image for im in ims[1:]])
    finally:
        _close(ims)
    assert got.shape == (7, 4) and got.dtype == np.float32
    for k, (q, o) in enumerate(zip(got, oracle)):
        measured("roll %s %s pair %d" % (K.CASE_IDS[R.GPU_CASES.index(case)], fmt, k), dangle=abs(q[0] - o["angle"]), dpeak=abs(q[1] - o["peak"]),
                 dcoarse=abs(q[2] - o["peak_coarse"]), oracle_gap=o["gap"] / o["peak_coarse"], true=true[k], got=q[0],
                 bar_angle=bars["angle"], bar_peak=bars["peak"], bar_coarse=bars["peak_coarse"])
    for k, (q, o) in enumerate(zip(got, oracle)):
        assert q[3] == 0.0
        cells = [o["peak_coarse"]] if o["gap"] >= K.GAP_FOR_SAME_CELL * o["peak_coarse"] else [o["peak_coarse"]] + list(o["next_cells"])
        assert min(abs(q[2] - c) for c in cells) <= bars["peak_coarse"], (k, q, o)      # the coarse cell
        assert abs(q[0] - o["angle"]) <= bars["angle"], (k, q, o)
        assert abs(q[1] - o["peak"]) <= bars["peak"], (k, q, o)


def test_whole_band_wraps_the_columns():
    """band = 1 at 80 x 48, window 64 x 32: rho_max = n, so the band's columns -cx - 1 .. cx + 1 = -65 .. 65 are more than the 128
    bins of a padded row and wrap modulo it (three bins stored twice, column pairs whose partners alias), and the samples at
    theta = 0 read the Nyquist column and the one beyond.  Held to the oracle at the same band, with bars derived as everywhere:
    four times the complex64 oracle's difference to the complex128 oracle over these seven pairs."""
    case = R.GPU_CASES[0]
    W, H, window, d = case
    ref, moved, _ = K.scene(case)
    g = R.geometry(W, H, window, d, band=1.0)
    assert g["rho_max"] == g["n"] == 32
    oracle = [R.estimate(ref, cur, g) for cur in moved]
    single = [R.estimate(ref, cur, g, True) for cur in moved]
    bars = {k: 4.0 * max(abs(a[k] - b[k]) for a, b in zip(oracle, single)) for k in ("angle", "peak", "peak_coarse")}
    ims = _images(case, "rgb8", [ref] + list(moved))
    try:
        with _roller(case, "rgb8", band=1.0) as ro:
            assert (ro.info["rho_min"], ro.info["rho_max"]) == (g["rho_min"], g["rho_max"])
            got = ro.angles(ims[0].image, [im.image for im in ims[1:]])
    finally:
        _close(ims)
    for k, (q, o) in enumerate(zip(got, oracle)):
        measured("roll band 1 pair %d" % k, dangle=abs(q[0] - o["angle"]), dpeak=abs(q[1] - o["peak"]), dcoarse=abs(q[2] - o["peak_coarse"]),
                 oracle_gap=o["gap"] / o["peak_coarse"], bar_angle=bars["angle"], bar_peak=bars["peak"], bar_coarse=bars["peak_coarse"])
    for k, (q, o) in enumerate(zip(got, oracle)):
        assert o["gap"] >= K.GAP_FOR_SAME_CELL * o["peak_coarse"], (k, o)
        assert abs(q[2] - o["peak_coarse"]) <= bars["peak_coarse"] and abs(q[0] - o["angle"]) <= bars["angle"] and abs(q[1] - o["peak"]) <= bars["peak"], (k, q, o)


# ---------------------------------------------------------------- 2. layouts, batches, containment
@pytest.mark.parametrize("fmt", list(K.FORMATS))
def test_strides_unaligned_planes_batches_and_guards(fmt):
    """160 x 160: dense frames; then rows and planes with padding at an address that is no multiple of the element size (planes
    assembled from bytes; 8-bit rows at an odd address) -- the same bytes; five pairs on an estimator with max_batch = 2 (chunks of
    2, 2 and 1) against one call per pair, and the call a second time -- the same bytes; every guard byte around angles_device and
    every byte of padding untouched, the frames unchanged; then on a stream of its own, read back on that stream."""
    import vkresample_amd as v
    case = R.GPU_CASES[1]
    ref, moved, _ = K.scene(case)
    frames = [ref] + list(moved[:5])
    dense = _images(case, fmt, frames)
    odd = _images(case, fmt, frames, padded=True, base=GUARD + 1)
    res = _Result(5)
    try:
        with _roller(case, fmt, max_batch=2) as ro:
            before = [im.buf.download() for im in odd]
            ro.angles_device(dense[0].image, [im.image for im in dense[1:]], res.ptr)
            a, clean = res.read()
            assert clean
            ro.angles_device(dense[0].image, [im.image for im in dense[1:]], res.ptr)
            again, clean = res.read()
            assert clean and a.tobytes() == again.tobytes()
            ro.angles_device(odd[0].image, [im.image for im in odd[1:]], res.ptr)
            b, clean = res.read()
            assert clean and a.tobytes() == b.tobytes()
            assert all((im.buf.download() == x).all() for im, x in zip(odd, before))
            singles = np.concatenate([ro.angles(dense[0].image, [dense[k + 1].image]) for k in range(5)])
            assert singles.tobytes() == a.tobytes()
            with v.Stream(0) as st:
                res.buf.upload(np.full(2 * GUARD + 16 * 5, FILL, np.uint8), stream=st)
                ro.angles_device(odd[0].image, [im.image for im in odd[1:]], res.ptr, st)
                c, clean = res.read(st)
            assert clean and a.tobytes() == c.tobytes()
        assert np.abs(a[1:, 0]).min() > 1e-3 and (a[:, 3] == 0).all()      # (the frames did turn)
    finally:
        _close(dense + odd)
        res.close()


# ---------------------------------------------------------------- 3. known answers
@pytest.mark.parametrize("fmt", list(K.FORMATS))
def test_black_pair_gives_the_tie_rule(fmt):
    """two black frames: R = 0, the coarse argmax is cell 0 and the fine argmax its first point: angle = -pi / n_theta, peaks 0"""
    case = R.GPU_CASES[0]
    black = np.zeros((case[1], case[0], 3), np.uint8)
    ims = _images(case, fmt, [black, black])
    try:
        with _roller(case, fmt) as ro:
            got = ro.angles(ims[0].image, [ims[1].image, ims[0].image])
            nt = ro.info["angles"]
    finally:
        _close(ims)
    for q in got:
        assert q[0] == np.float32(np.float32(np.pi) * np.float32(-1.0) / np.float32(nt)) and q[1] == 0.0 and q[2] == 0.0 and q[3] == 0.0, got


@pytest.mark.parametrize("case", R.ACCURACY_CASES, ids=K.CASE_IDS[1:])
def test_translation_alone_and_known_angles(case):
    """pair 0 of every scene is moved by (0.8, -1.4) decimated pixels and not turned: |angle| below the window's accuracy bar
    (roll_oracle.ACCURACY_BAR) -- the estimate reads magnitudes only; and every turned pair comes back within that bar of the TRUE
    angle, whatever the oracle says; a frame against itself gives 0 and peaks of 1 within the fp32 bars"""
    bars = K.bars()
    ref, moved, true = K.scene(case)
    ims = _images(case, "rgb8", [ref] + list(moved))
    try:
        with _roller(case, "rgb8") as ro:
            got = ro.angles(ims[0].image, [im.image for im in ims[1:]] + [ims[0].image])
    finally:
        _close(ims)
    bar = R.ACCURACY_BAR[case[:2]]
    for q, a in zip(got, true):
        measured("roll accuracy %dx%d" % case[:2], true=a, error=q[0] - a, peak=q[1], bar=bar)
    assert true[0] == 0.0 and abs(got[0][0]) <= bar
    for q, a in zip(got, true):
        assert abs(q[0] - a) <= bar and q[1] >= 0.5, (q, a)
    same = got[7]
    assert abs(same[0]) <= bars["angle"] and abs(same[1] - 1.0) <= bars["peak"] and abs(same[2] - 1.0) <= bars["peak_coarse"], same


# ---------------------------------------------------------------- 4. validation
def test_validation_before_any_launch():
    """each refused call returns FFTUP_E_INVALID_ARG, names the rule, and leaves angles_device untouched (all 0xA5)"""
    from vkresample_amd import _lib
    lib = _lib.load()
    case = R.GPU_CASES[0]
    W, H = case[:2]
    ref = K.scene(case)[0]
    ims = _images(case, "rgb8", [ref])
    res = _Result(1)
    hostmem = np.zeros(3 * W * H + 16, dtype=np.uint8)
    try:
        with _roller(case, "rgb8") as ro:
            a = (_lib.DeviceImageDesc * 1)(ims[0].image.desc())
            host_in = (_lib.DeviceImageDesc * 1)(_lib.DeviceImageDesc(hostmem.ctypes.data, RGB8, 3 * W, 0))
            short = (_lib.DeviceImageDesc * 1)(_lib.DeviceImageDesc(ims[0].image.ptr, RGB8, 3 * W - 1, 0))
            calls = [
                ((a, a, 1, None), "angles_device is null"),
                ((a, a, 0, res.ptr), "n_pairs must be > 0"),
                ((None, a, 1, res.ptr), "null image array"),
                ((host_in, a, 1, res.ptr), "ref[0].data is not device memory"),
                ((a, short, 1, res.ptr), "cur[0].row_stride_bytes %d is below one row" % (3 * W - 1)),
                ((a, a, 1, res.ptr + 2), "angles_device is not a multiple of 4 bytes"),
                ((a, a, 1, hostmem.ctypes.data), "angles_device is not device memory"),
            ]
            for args, piece in calls:
                code = lib.fftup_roll_angles(ro._h, args[0], args[1], args[2], args[3], None)
                text = lib.fftup_last_error().decode()
                assert code == 1 and piece in text, (code, text, piece)
            raw, clean = res.read()
            assert clean and (raw.view(np.uint8) == FILL).all()
    finally:
        _close(ims)
        res.close()
