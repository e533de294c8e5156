"""GPU: the five kernels of fftup_align_shifts (csrc/kernels_align.hpp) against the fp64 oracle (tests/align_oracle.py) at the edges of
the aligner's geometry -- tests/align_edge_cases.py has the table, the bars and their reasons; tests/test_align_edge_oracle.py proves
on the CPU what these tests take for granted (the oracle's coarse gaps, the pairs that qualify for the tight bar, the literals of the
bars, the geometry of every row), so no assert below is ever skipped on a condition.

What each test reaches that tests/test_gpu_align.py does not:
    test_edge_parity                      band 1 (Kx = n_x, the self-paired column n_x / 2, index -n/2 at Rb 0), band 0.99, 0.25 and
                                          0.1, kappa 4 and 64, n_y > n_x, n = 16 and n = 1024 on either axis, d = 4 and 8, a coarse
                                          peak a quarter window away
    test_forty_five_pairs_in_one_call     pair0 = 16 and 32 in k_align_rows, a second chunk behind a chunk of 40
    test_result_pointer_at_4_mod_16       the scalar store of the result in k_align_fine_y
    test_planes_at_an_odd_byte_address    AlignImage kinds 3 and 4 (align_px assembles each value from bytes)
    test_no_signal                        R = 0 everywhere: the tie rule of both argmaxes, and a dead pair beside a live one"""
import numpy as np
import pytest

import align_edge_cases as EC
import align_oracle as AO
from devimage import FILL, GUARD, PLANAR, RGB8, Image
from paritylib import measured

pytestmark = pytest.mark.gpu

# name -> (descriptor format, precision of the aligner, bytes per element); the conversions are EC.FORMATS'
FORMATS = {"rgb8": (RGB8, 0, 1), "planar_f32": (PLANAR, 0, 4), "planar_f16": (PLANAR, 2, 2)}

_clips, _oracles, _long = {}, {}, {}


def _clip(name):
    if name not in _clips:
        _clips[name] = EC.row_clip(EC.row(name))
    return _clips[name]


def _oracle(name, fmt):
    """the fp64 estimates of the row's pairs on the values the library reads in this format: computed once, left unchanged"""
    if (name, fmt) not in _oracles:
        conv = EC.FORMATS[fmt]
        ref, moved, _ = _clip(name)
        g = EC.geometry(EC.row(name))
        _oracles[(name, fmt)] = [AO.estimate(conv(ref), conv(cur), g) for cur in moved]
    return _oracles[(name, fmt)]


def _images(W, H, fmt, frames, padded=False, base=GUARD):
    dfmt, _, esz = FORMATS[fmt]
    return [Image(dfmt, W, H, esz, padded, base, EC.FORMATS[fmt](f)) for f in frames]


def _aligner(W, H, fmt, window, d, band=0.0, upsample=0, **kw):
    import vkresample_amd as v
    return v.Aligner(W, H, FORMATS[fmt][1], window=window, decimate=d, band=band, upsample=upsample, **kw)


def _close(things):
    for t in things:
        t.close()


def _assert_geometry(al, g):
    got = tuple(al.info[k] for k in ("window_w", "window_h", "decimate", "upsample", "band_kx", "band_ky", "crop_x", "crop_y"))
    assert got == (g["nx"], g["ny"], g["d"], g["kappa"], g["band_kx"], g["band_ky"], g["crop_x"], g["crop_y"]), (got, g)


def _assert_pair(tag, got, o, d, kappa, tight=None):
    """one fftup_shift against its oracle: the figures, then the bars of tests/align_edge_cases.py"""
    ddx, ddy = abs(got[0] - o["dx"]), abs(got[1] - o["dy"])
    q = EC.qualifies(o)
    measured(tag, ddx=ddx, ddy=ddy, dpeak=abs(got[2] - o["peak"]), dcoarse=abs(got[3] - o["peak_coarse"]), oracle_gap=o["gap"],
             qualifies=q, tight_bar=tight if tight is not None else float("nan"), vertex_x=o["dx_"], vertex_y=o["dy_"])
    assert abs(got[3] - o["peak_coarse"]) <= EC.EDGE_PEAK_BAR, (tag, got, o)            # ... which also says: the same coarse cell
    assert ddx <= d / kappa and ddy <= d / kappa, (tag, got, o)
    assert abs(got[2] - o["peak"]) <= EC.EDGE_PEAK_BAR, (tag, got, o)
    if tight is not None and q:
        assert ddx <= tight and ddy <= tight, (tag, got, o, tight)


# ---------------------------------------------------------------- a. parity per row and format
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", EC.NAMES)
def test_edge_parity(name, fmt):
    """all of a row's pairs in one call with max_batch = 3.  Bars: peak and peak_coarse within EDGE_PEAK_BAR of the oracle, dx and dy
    within d / kappa, and within the row's tight bar for the pairs that qualify (tests/align_edge_cases.py).  Measured on an MI355X
    (profiles/align_edges_measured.txt): dx, dy at most 0.30 of the row's tight bar, on every pair (x1024: 2.9e-5 px of 1.28e-4;
    band1: 2.4e-6 of 8e-6); peak and peak_coarse at most 7.8e-7 of 1.25e-6 (band1)."""
    r = EC.row(name)
    _, W, H, window, d, band, kappa = r[:7]
    g = EC.geometry(r)
    ref, moved, _ = _clip(name)
    oracle = _oracle(name, fmt)
    ims = _images(W, H, fmt, [ref] + moved)
    try:
        with _aligner(W, H, fmt, window, d, band, kappa, max_batch=3) as al:
            _assert_geometry(al, g)
            got = al.shifts(ims[0].image, [im.image for im in ims[1:]])
    finally:
        _close(ims)
    assert got.shape == (len(moved), 4) and got.dtype == np.float32
    for k, (s, o) in enumerate(zip(got, oracle)):
        _assert_pair("align edge %s %s pair %d" % (name, fmt, k), s, o, d, kappa, EC.tight_bar(r))


# ---------------------------------------------------------------- b. forty-five pairs
@pytest.mark.parametrize("fmt", ["rgb8", "planar_f16"])
def test_forty_five_pairs_in_one_call(fmt):
    """45 ordered pairs of the eight frames of AO.CASES[0] in ONE call at max_batch = 40: the first chunk's rows go in launches of
    16, 16 and 8 (pair0 = 0, 16, 32 in k_align_rows), a chunk of 5 follows in the same buffers.  Bit for bit the 45 single-pair calls
    on the same aligner, and every pair within the parity bars of its own oracle: d / kappa and EDGE_PEAK_BAR (the tight shift bar
    is a figure per row of the table, and these pairs are none).  Measured: dx, dy within 3.9e-6 px, peaks within 6.6e-7."""
    W, H, window, d = EC.LONG_CASE
    g = AO.geometry(W, H, window, d)
    if fmt not in _long:
        conv = EC.FORMATS[fmt]
        fr = [conv(f) for f in EC.long_frames()]
        _long[fmt] = [AO.estimate(fr[a], fr[b], g) for (a, b) in EC.LONG_PAIRS]
    oracle = _long[fmt]
    ims = _images(W, H, fmt, EC.long_frames())
    try:
        with _aligner(W, H, fmt, window, d, max_batch=EC.LONG_MAX_BATCH) as al:
            _assert_geometry(al, g)
            desc = [im.image for im in ims]
            refs, curs = [desc[a] for (a, _) in EC.LONG_PAIRS], [desc[b] for (_, b) in EC.LONG_PAIRS]
            got = al.shifts(refs, curs)
            single = np.concatenate([al.shifts([r], [c]) for r, c in zip(refs, curs)])
    finally:
        _close(ims)
    assert got.shape == (45, 4) and len(EC.LONG_PAIRS) == 45
    differ = [k for k in range(45) if got[k].tobytes() != single[k].tobytes()]
    measured("align 45 pairs %s" % fmt, pairs_that_differ_from_their_single_call=len(differ))
    for k, (s, o) in enumerate(zip(got, oracle)):
        _assert_pair("align 45 pairs %s pair %d (%d, %d)" % ((fmt, k) + EC.LONG_PAIRS[k]), s, o, d, g["kappa"])
    assert not differ, (differ, got[differ], single[differ])


# ---------------------------------------------------------------- c. the result at 4 mod 16
class _Result:
    """n fftup_shift in device memory `offset` bytes behind a guard band of 0xA5, another band behind them"""

    def __init__(self, n, offset=0):
        import vkresample_amd as v
        self.n, self.lo = n, GUARD + offset
        self.size = 2 * GUARD + 16 * n + 16
        self.buf = v.DeviceBuffer(self.size)
        self.buf.upload(np.full(self.size, FILL, np.uint8))
        self.ptr = self.buf.ptr + self.lo

    def read(self):
        """-> ((n, 4) float32, True if every byte in front of and behind the results is untouched)"""
        raw = self.buf.download()
        hi = self.lo + 16 * self.n
        return raw[self.lo:hi].copy().view(np.float32).reshape(self.n, 4), bool((raw[:self.lo] == FILL).all() and (raw[hi:] == FILL).all())

    def close(self):
        self.buf.close()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_result_pointer_at_4_mod_16(fmt):
    """three pairs at max_batch = 2 into a result array 4 bytes past a 16-byte boundary (the API asks for 4-byte alignment only), so
    that the second chunk's pointer is misaligned too: the bytes of the aligned call, both guard bands untouched"""
    W, H, window, d = AO.CASES[0]
    ref, moved, _ = AO.case_clip(W, H, d)
    ims = _images(W, H, fmt, [ref] + moved[:3])
    res = [_Result(3, 0), _Result(3, 4)]
    try:
        assert res[0].ptr % 16 == 0 and res[1].ptr % 16 == 4
        with _aligner(W, H, fmt, window, d, max_batch=2) as al:
            for r in res:
                al.shifts_device(ims[0].image, [im.image for im in ims[1:]], r.ptr)
            (a, a_ok), (b, b_ok) = res[0].read(), res[1].read()
    finally:
        _close(ims + res)
    measured("align result at 4 mod 16 %s" % fmt, values_that_differ=int((a.view(np.uint32) != b.view(np.uint32)).sum()), guards_ok=a_ok and b_ok)
    assert a_ok and b_ok
    assert a.tobytes() == b.tobytes(), (a, b)
    assert np.abs(a[:, :2]).max() > 0.5 and (a[:, 2] > 0.5).all()              # (estimates, not fill)


# ---------------------------------------------------------------- d. planes at an odd byte address
@pytest.mark.parametrize("padded", [False, True], ids=["dense", "padded"])
@pytest.mark.parametrize("fmt", ["planar_f32", "planar_f16"])
def test_planes_at_an_odd_byte_address(fmt, padded):
    """float and half planes one byte past the guard band (AlignImage kinds 3 and 4): the results of the aligned planes bit for bit,
    every guard and padding byte untouched, the frames unchanged"""
    W, H, window, d = AO.CASES[0]
    ref, moved, _ = AO.case_clip(W, H, d)
    frames = [ref] + moved[:3]
    even = _images(W, H, fmt, frames, padded)
    odd = _images(W, H, fmt, frames, padded, base=GUARD + 1)
    try:
        assert all(im.image.ptr % 2 == 1 for im in odd) and all(im.image.ptr % 4 == 0 for im in even)
        with _aligner(W, H, fmt, window, d) as al:
            a = al.shifts(even[0].image, [im.image for im in even[1:]])
            b = al.shifts(odd[0].image, [im.image for im in odd[1:]])
        measured("align odd address %s %s" % (fmt, "padded" if padded else "dense"), values_that_differ=int((a.view(np.uint32) != b.view(np.uint32)).sum()))
        assert a.tobytes() == b.tobytes(), (a, b)
        assert np.abs(a[:, :2]).max() > 0.5 and (a[:, 2] > 0.5).all()
        for im, f in zip(even + odd, frames + frames):
            pixels, guards = im.read()
            assert guards and pixels.tobytes() == np.ascontiguousarray(EC.FORMATS[fmt](f)).tobytes()
    finally:
        _close(even + odd)


# ---------------------------------------------------------------- e. no signal
@pytest.mark.parametrize("fmt", ["rgb8", "planar_f32"])
@pytest.mark.parametrize("name", EC.NO_SIGNAL_ROWS)
def test_no_signal(name, fmt):
    """black-black, black-frame and frame-black: P[0,0] = 0, so R = 0 everywhere, peak and peak_coarse are exactly 0 and the tie rule
    of include/fftup.h sends both argmaxes to index 0 -- dx = dy = -d, the oracle's value (tests/align_edge_cases.py has the
    argument, tests/test_align_edge_oracle.py the oracle's own result for the three pairs).  An ordinary fourth pair in the same call
    keeps the bytes of its single call: a dead pair does not leak into its neighbour.
    This test found k_align_cols correlating rounding: with a floor of 1e-9 |P[0,0]| = 0 alone, the residue that the packed
    transform leaves in the black frame's bins passed as unit phasors -- black-frame at 80 x 48 returned dx 25.6, dy 5.07, peak
    0.137 (d4: dx 73.6, peak 0.151).  Since the kernel treats P[0,0] = 0 as no signal: (-d, -d, 0, 0) in all four cases."""
    W, H, window, d, band, kappa, ref, cur, black = EC.no_signal_case(name)
    ims = _images(W, H, fmt, [ref, cur, black])
    try:
        with _aligner(W, H, fmt, window, d, band, kappa) as al:
            r, c, b = (im.image for im in ims)
            got = al.shifts([b, b, r, r], [b, r, b, c])
            alone = al.shifts([r], [c])
    finally:
        _close(ims)
    for k, tag in enumerate(("black-black", "black-frame", "frame-black")):
        measured("align no signal %s %s %s" % (name, fmt, tag), dx=got[k][0], dy=got[k][1], peak=got[k][2], peak_coarse=got[k][3])
    measured("align no signal %s %s live pair" % (name, fmt), dx=got[3][0], dy=got[3][1], peak=got[3][2], same_as_alone=got[3].tobytes() == alone[0].tobytes())
    for k in range(3):
        assert tuple(float(x) for x in got[k]) == EC.dead_result(d), (k, got)
    assert got[3].tobytes() == alone[0].tobytes(), (got, alone)
    assert abs(got[3][0]) > 0.5 * d and got[3][2] > 0.5                         # (the live pair is one)
