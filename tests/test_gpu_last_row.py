"""GPU: the last output row, uH-1, of every kernel that sharpens -- against the oracle's definition of it.

The reference's sharpen shader has no upper clamp: on the last row its S, SE and E taps read the padding behind the plane (quirk
B5), so the reference's own last row is undefined.  This project defines it: a read at or past the end of a plane takes "same
column, last written row" (oracle/fftup_oracle.c: `while (f >= plane) f -= uW`) -- rows past uH-1 are row uH-1, and the wrapped
right neighbour of (uH-1, uW-1), one element past the plane, folds onto (uH-1, 0).  The size-generic kernels implement that
literally, the fused C2R+sharpen kernels through a duplicated last row pair, a corner sample switched off for the last strip and a
deferred pixel; the other GPU files compare whole images, this one aims at the bottom edge and at each kernel that computes it.

Per case and frame, on rows uH-3 .. uH-1 (a failure names the last row's error beside that of the two rows above it, and the two
corner pixels (uH-1, 0) and (uH-1, uW-1) on their own):
  * the planes and the 8-bit image against the full oracle (oraclelib.upscale_rgb8, or the family's oracle and oraclelib.sharpen);
  * the planes against oraclelib.sharpen applied to the last rows of the DEVICE's own pre-sharpen image -- two rows decide the last
    output row (checked on the CPU: sharpen(pre[:, -2:])[:, -1] is sharpen(pre)[:, -1] bit for bit), four are passed so that the
    rows above come out of the same call.  This separates the sharpen from the transforms and costs nothing at 4096x2048.
Frames: natural-like ("N"), uniform noise ("U"), "E": a natural-like frame whose last input row is black and whose second-to-last
is white, and "G": the same with the two rows at 64 and 192.  "G" is the frame on which a kernel that reads row uH-2 or row 0 where
the definition says uH-1 is off by 0.03 .. 0.2 in every case of this file (computed with the oracle).  "E" is not always: where the
last output rows are black the 3x3 minimum is 0, the filter's scale sqrt(min) vanishes and the output is the centre tap whatever
the other taps are (45x21 -u 2 and 50x32 -> 63x32 move by 1e-9 under either mistake); on the other plans it moves by 2e-3 .. 0.1.

No bar is new; every one is a bar tests/test_gpu_parity.py states for the rows above (and the family modules repeat):
  -p 0: output against the oracle max 2e-5 and relative L2 5e-6 on natural-like frames, max 5e-4 on uniform noise; against the
        sharpen of the device's own pre-sharpen image 3e-6 / 1e-4 (test_fp32_parity_small), on two-launch and on fused plans
        alike.  A fused plan's pre-sharpen tap is a C2R of its own, equal to the rows the fused kernel sharpens up to fp32
        rounding only, so its figures are the larger ones: up to a third of the bar (profiles/last_row_parity.txt).
        The non-R2C plans have no such comparison: their tap is the real part of a complex image whose modulus is sharpened.
        Frame "E" takes the uniform-noise bars: its white row clamps at 1 and its black row sits at 0, the two ends where the
        filter's sqrt has unbounded slope -- the reason the module docstring of test_gpu_parity.py gives for those bars.  Frame
        "G" stays away from both ends and takes the bars of natural-like frames.
        8-bit image: one code.
  -p 1: 1e-9 (test_fp64_parity), 8-bit image one code.
  -p 2: pre-sharpen within one binary16 ulp, output max 8e-3, 8-bit image two codes; bit for bit against the sharpen of the device's
        own image on the FFT path's two-launch plan (FFTUP_FLAG_UNFUSED_SHARPEN, as test_fp16_parity_small asserts above the last
        row); on fused plans the fused kernel's packed-binary16 sharpen differs from the exactly rounded sequence by an ulp here and
        there (test_fused_sharpen_equals_unfused) and the 8e-3 holds.  The one-ulp bound on R needs the oracle's image: asserted
        wherever the oracle runs; for 640x480 and 2048x1024 its transforms alone run, on one frame (0.4 s at 4096x2048).  The bars on the FRACTION of differing values (1 % of R, 2 % of the output) mean nothing on one row: they are asserted
        on the counts pooled over all -p 2 cases (test_pooled_fp16_fractions), as tests/test_gpu_family_sweep.py does for its tiny
        outputs.
What each case reaches is read off the plan (description with factorization and threads, tuned, specialised_at_plan_time,
kernel_names, u8_store) and asserted; so is the strip length in force, from the halo factor (pairs + 1) / pairs that
kernel_min_bytes[2] carries -- a pairs_per_strip the library did not parse would otherwise repeat the default cut unnoticed.
The planner accepts no -p 1 plan with an odd output width (FFTUP_FLAG_ODD_SIZE and fftup_plan_create_size plans exist for -p 0 and
-p 2 only), so the element-wise branch of k_sharpen_f64 has no case here; 20x12 -p 1 runs its even-width branch.

Measured on an MI355X: profiles/last_row_parity.txt (pytest -s of this file).
"""
import contextlib
import functools
import io
import os

import numpy as np
import pytest

import oraclelib as O
from paritylib import measured, rel_l2, within_one_half_ulp
from test_gpu_parity import _knobs_lib

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _kind_frame(kind, W, H, seed):
    """(read-only: the cases of one size share their frames)"""
    from vkresample_amd import synth
    f = synth.frame(seed, W, H, kind if kind in "NU" else "N").copy()
    if kind in "EG":
        f[-1], f[-2] = (0, 255) if kind == "E" else (64, 192)
    f.setflags(write=False)
    return f


@contextlib.contextmanager
def _knobs(text):
    """FFTUP_EXPERIMENT (read at plan creation) in the test build of the library, as test_fused_output_independent_of_strip_length"""
    env = {"FFTUP_EXPERIMENT": text, "FFTUP_LIBRARY": _knobs_lib()} if text else {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _store_u8(x):
    """the oracle's saturating store (orc_store_u8): trunc(255 x) in [0, 255]"""
    return np.clip(np.trunc(255.0 * np.nan_to_num(x)), 0, 255).astype(np.uint8)


def _bars(precision, kind, bit_exact):
    """(max against the oracle, relative L2 against the oracle or None, max against the sharpen of the device's own image, codes)"""
    if precision == 1:
        return 1e-9, None, 1e-9, 1
    if precision == 2:
        return 8e-3, None, (0.0 if bit_exact else 8e-3), 2
    if kind in "NG":
        return 2e-5, 5e-6, 3e-6, 1
    return 5e-4, None, 1e-4, 1


def _rows(tag, got, ref, bar, l2_bar=None):
    """got, ref: rows uH-3, uH-2, uH-1 of the three planes"""
    d = np.abs(got - ref)
    above, last, left, right = d[:, :2].max(), d[:, 2].max(), d[:, 2, 0].max(), d[:, 2, -1].max()
    vals = dict(last_row=last, rows_above=above, corner_left=left, corner_right=right, bar=bar)
    if l2_bar is not None:          # (printed where it is asserted: on a black row it is a ratio of two roundings)
        l2 = vals["last_row_l2"] = rel_l2(got[:, 2], ref[:, 2])
    measured(tag, **vals)
    assert left <= bar, "%s: pixel (uH-1, 0) off by %g (bar %g; rows uH-3, uH-2: %g)" % (tag, left, bar, above)
    assert right <= bar, ("%s: pixel (uH-1, uW-1), whose E, NE and SE taps all fold onto (uH-1, 0), off by %g (bar %g; rows uH-3, uH-2: %g)"
                          % (tag, right, bar, above))
    assert last <= bar, "%s: last row off by %g at column %d (bar %g; rows uH-3, uH-2: %g)" % (tag, last, int(d[:, 2].max(axis=0).argmax()), bar, above)
    assert above <= bar, "%s: rows uH-3, uH-2 off by %g (bar %g; last row: %g)" % (tag, above, bar, last)
    if l2_bar is not None:
        assert l2 <= l2_bar, "%s: last row relative L2 %g (bar %g)" % (tag, l2, l2_bar)


def _codes(tag, got, ref, bar):
    """got, ref: rows uH-3 .. uH-1 of two 8-bit images"""
    d = np.abs(got.astype(int) - ref.astype(int))
    print("MEASURED %s: last_row max %d differing %d of %d  rows_above max %d" % (tag, d[2].max(), int((d[2] != 0).sum()), d[2].size, d[:2].max()))
    assert d[2].max() <= bar, "%s: last row of the 8-bit image off by %d codes (rows above: %d)" % (tag, d[2].max(), d[:2].max())
    assert d[:2].max() <= bar, "%s: rows uH-3, uH-2 of the 8-bit image off by %d codes" % (tag, d[:2].max())


# ---------------------------------------------------------------------------------------------------------------- what a case reaches
def _generic(up):
    assert up.description.startswith("size-generic kernels (") and not up.tuned and up.kernel_names[3] == "sharpen", (up.description, up.kernel_names)


def _f64(up):
    assert up.description.startswith("size-generic kernels (") and ", double" in up.description and up.kernel_names[3] == "sharpen", up.description


def _aot(up):
    assert up.description.startswith("ahead-of-time power-of-two") and "fused C2R+sharpen on" in up.description, up.description
    assert up.tuned and not up.specialised_at_plan_time and up.kernel_names[2:] == ["row_c2r_sharpen", "-"], up.kernel_names


def _jit(fused):
    """fused: factorization and threads of the fused kernel as the plan describes them"""
    def check(up):
        assert up.tuned and up.specialised_at_plan_time and up.kernel_names[3] == "-", (up.description, up.kernel_names)
        assert "fused " + fused + " " in up.description, up.description
    return check


def _pairs_per_strip(up):
    """the strip length of a fused planes plan, from its byte counts: kernel_alg_bytes[2] = S2 + 2 R + out, kernel_min_bytes[2] =
    S2 (pairs + 1) / pairs + out, R = out = the three output planes"""
    o = 3.0 * up.out_width * up.out_height * np.dtype(up._dtype).itemsize
    S2 = up.kernel_alg_bytes[2] - 3.0 * o
    return S2 / (up.kernel_min_bytes[2] - o - S2)


def _cplx(up):
    assert up.description.startswith("size-generic kernels, non-R2C path") and "four steps" not in up.description, up.description
    assert up.kernel_names == ["row_c2c", "col_fwd_pad_inv", "row_c2c_inv", "sharpen"] and not up.tuned, up.kernel_names


def _four_step(up):
    assert "non-R2C path" in up.description and "inverse rows in four steps 128*144" in up.description and up.kernel_names[3] == "sharpen", up.description


def _named(prefix, *parts):
    def check(up):
        assert up.description.startswith(prefix) and all(s in up.description for s in parts), up.description
        assert not up.tuned and up.num_kernels == 4 and up.kernel_names[3] == "sharpen", up.kernel_names
    return check


# ---------------------------------------------------------------------------------------------------------------- the cases
SEED = {"N": 900, "U": 901, "E": 902, "G": 903}


class Case:
    def __init__(self, make, reaches, precision, u_e, oracle, kinds="NUEG", knobs=None, two_launch=False, bit_exact=False, own=True, oracle_kinds=None, pairs=None,
                 pre_oracle=None, pre_kinds=""):
        """two_launch: the pre-sharpen image is exactly what the sharpen kernel read; bit_exact: ... and at -p 2 the output is the oracle's
        sharpen of it bit for bit (test_fp16_parity_small asserts that of the FFT path's two-launch plans, nobody of the families);
        own: compare with the sharpen of the device's own pre-sharpen rows; oracle_kinds: the frames that get a full oracle run as well
        (default: all of `kinds`; the large frames: the most sensitive one); pairs: the strip length the plan must report (a number, or
        a function of the plan); pre_oracle, pre_kinds: the oracle's pre-sharpen image alone, for the -p 2 bound on R of these frames"""
        self.make, self.reaches, self.precision, self.u_e, self.oracle = make, reaches, precision, u_e, oracle
        self.kinds, self.knobs, self.two_launch, self.bit_exact, self.own = kinds, knobs, two_launch, bit_exact, own
        self.oracle_kinds = (kinds if oracle_kinds is None else oracle_kinds) if oracle is not None else ""
        self.pairs, self.pre_oracle, self.pre_kinds = pairs, pre_oracle, pre_kinds


@functools.lru_cache(maxsize=None)
def _fft_oracle(W, H, u, precision, kind):
    """(pre-sharpen image, rows uH-3 .. uH-1 of the output and of the 8-bit image) by the full oracle; computed once per frame --
    the cases that differ in their strip cuts share it"""
    opre, oout, ou8 = O.upscale_rgb8(_kind_frame(kind, W, H, SEED[kind]), u, precision, 0.2)
    return opre, oout[:, -3:].copy(), ou8[-3:].copy()


@functools.lru_cache(maxsize=None)
def _fft_pre_oracle(W, H, u, precision, kind):
    return O.presharpen_rgb8(_kind_frame(kind, W, H, SEED[kind]), u, precision)


def _fft(W, H, u, precision, reaches, flags=0, ring=1, full=True, **kw):
    """a plan of fftup_plan_create on the periodic FFT path; full: compare with the full oracle too (not at 4096x2048, and not the
    slow binary16 sharpen of the oracle on large frames)"""
    def make():
        import vkresample_amd as v
        return v.Upscaler(W, H, u, precision, 0.2, 0, flags, ring)

    return Case(make, reaches, precision, u, functools.partial(_fft_oracle, W, H, u, precision) if full else None,
                pre_oracle=functools.partial(_fft_pre_oracle, W, H, u, precision), **kw), (W, H)


def _family(W, H, precision, u_e, make, reaches, R_of, **kw):
    """a plan of one of the resampling families: R_of(x) is the family's own oracle for the pre-sharpen image R of input planes x"""
    def oracle(kind):
        rgb = _kind_frame(kind, W, H, SEED[kind])
        R = R_of(O.load_lut(precision)[np.transpose(rgb, (2, 0, 1))])
        opre = R.astype(np.float16).astype(np.float64) if precision == 2 else R
        sh = O.sharpen(opre, u_e, precision, 0.2)
        return opre, sh[:, -3:], _store_u8(sh[:, -3:]).transpose(1, 2, 0)
    return Case(make, reaches, precision, u_e, oracle, kinds="NEG", two_launch=True, **kw), (W, H)


def _cases():
    import dct_oracle as D
    import downscale_oracle as S
    import exactsize_oracle as EX
    import oddsize_oracle as Q
    import test_gpu_anysize as A
    import test_gpu_dct as DC
    import test_gpu_downscale as DN
    import test_gpu_view as VW
    import view_oracle as V
    import vkresample_amd as v
    from oracle import ref_layout_emulation as RL
    G = v.FLAG_GENERIC_KERNELS | v.FLAG_UNFUSED_SHARPEN
    c = {}
    # size-generic k_sharpen: fp32, fp16, fp64 (two launches: the pre-sharpen image is what the sharpen read)
    c["generic 64x32 p0"] = _fft(64, 32, 2.0, 0, _generic, G, two_launch=True)
    c["generic 64x32 p2"] = _fft(64, 32, 2.0, 2, _generic, G, two_launch=True, bit_exact=True)
    c["generic 20x12 p1"] = _fft(20, 12, 2.0, 1, _f64, two_launch=True)
    # ahead-of-time power-of-two fused kernels (2048x1024: no full oracle run at that size)
    c["aot 512x256 p0"] = _fft(512, 256, 2.0, 0, _aot)
    c["aot 512x256 p2"] = _fft(512, 256, 2.0, 2, _aot)
    c["aot 1024x512 p0"] = _fft(1024, 512, 2.0, 0, _aot, kinds="UG", oracle_kinds="G")
    c["aot 2048x1024 p0"] = _fft(2048, 1024, 2.0, 0, _aot, full=False, kinds="UEG")
    c["aot 2048x1024 p2"] = _fft(2048, 1024, 2.0, 2, _aot, full=False, kinds="NG", pre_kinds="G")
    # fused kernels specialised at plan time, small sizes only (plan creation is what this file's time goes to): a four-stage plan such
    # as 1000x1000 has its whole image, last row included, compared in tests/test_gpu_jit.py
    c["jit 128x64 p0"] = _fft(128, 64, 2.0, 0, _jit("8*4*8 x128"))
    c["jit 128x64 p2"] = _fft(128, 64, 2.0, 2, _jit("8*4*8 x128"), v.FLAG_FUSE_U8_LOAD)
    c["jit 640x480 p0"] = _fft(640, 480, 2.0, 0, _jit("8*10*16 x256"))
    c["jit 640x480 p2"] = _fft(640, 480, 2.0, 2, _jit("8*10*16 x256"), v.FLAG_FUSE_U8_LOAD, full=False, kinds="NG", pre_kinds="G")
    c["jit 486x294 p0"] = _fft(486, 294, 2.0, 0, _jit("12*9*9 x192"))
    c["jit 720x576 p0"] = _fft(720, 576, 2.0, 0, _jit("8*12*15 x256"), kinds="NG", oracle_kinds="G")
    # factors other than 2: U - 1 residue transforms, k_col_pad (tests/test_gpu_jit.py: U_CASES)
    c["jit 640x480 u3 p0"] = _fft(640, 480, 3.0, 0, _jit("12*10*16 x256"), kinds="NEG", oracle_kinds="G")
    c["jit 1280x720 u1.5 p0"] = _fft(1280, 720, 1.5, 0, _jit("12*10*16 x256"), kinds="NG", full=False)
    # where the strips of the fused kernel are cut at the bottom: 1, 2, 3 pairs; 3 uH / 2 = 1440 pairs = 1439 + 1 -- the last strip
    # is its halo pair and the duplicated pair alone; ring = 3 (frames that overlap: one strip per compute unit, another default cut)
    for pairs in (1, 2, 3):
        kw = dict(knobs="pairs_per_strip=%d" % pairs, kinds="NG", pairs=pairs)
        c["aot 512x256 p0 pairs=%d" % pairs] = _fft(512, 256, 2.0, 0, _aot, **kw)
        c["aot 512x256 p2 pairs=%d" % pairs] = _fft(512, 256, 2.0, 2, _aot, **kw)
        c["jit 640x480 p0 pairs=%d" % pairs] = _fft(640, 480, 2.0, 0, _jit("8*10*16 x256"), **kw)
    assert (3 * 960 // 2) % 1439 == 1
    c["jit 640x480 p0 pairs=1439"] = _fft(640, 480, 2.0, 0, _jit("8*10*16 x256"), knobs="pairs_per_strip=1439", kinds="NEG", pairs=1439)

    def other_cut(up):
        """ring = 3: whatever the default cut of overlapping frames is on this device, it is not that of a plan without a ring"""
        with v.Upscaler(640, 480, 2.0, 0) as plain:
            return None if abs(_pairs_per_strip(plain) - _pairs_per_strip(up)) < 0.5 else _pairs_per_strip(up)
    c["jit 640x480 p0 ring=3"] = _fft(640, 480, 2.0, 0, _jit("8*10*16 x256"), ring=3, kinds="NEG", pairs=other_cut)
    # beyond the R2C limit: the complex sharpen, rows in one launch and in four steps
    # (the pre-sharpen tap is the real part of the complex image whose modulus the sharpen takes, and the imaginary part is no
    # rounding noise on this path: the tap alone is no reference for the output)
    c["non-R2C 4608x16 p0"] = _fft(4608, 16, 2.0, 0, _cplx, own=False)
    c["four-step 9216x8 p0"] = _fft(9216, 8, 2.0, 0, _four_step, own=False)

    # odd output height, odd output width, both (binary16), odd input sizes
    def exact(W, H, uW, uH, p):
        return _family(W, H, p, EX.effective_factor(W, H, uW, uH), lambda: v.Upscaler.to_size(W, H, uW, uH, p, 0.2, 0, v.FLAG_ODD_SIZE),
                       _named("exact size:", "rows %d->%d" % (W, uW), "columns %d->%d" % (H, uH)), lambda x: EX.resample_R(x, uW, uH, EX.ALIGN_CORNER))
    c["exact 50x32->50x35 p0 (odd uH)"] = exact(50, 32, 50, 35, 0)
    c["exact 50x32->63x32 p0 (odd uW)"] = exact(50, 32, 63, 32, 0)
    c["exact 50x32->63x35 p2 (odd both)"] = exact(50, 32, 63, 35, 2)
    c["odd 45x21 u2 p0"] = _family(45, 21, 0, 2.0, lambda: v.Upscaler(45, 21, 2.0, 0, 0.2, 0, v.FLAG_ODD_SIZE), _named("odd sizes:", "rows 45->90", "columns 21->42"),
                                   lambda x: Q.resample_R(x, 90, 42))
    # the smallest case of each family's list
    W, H, u = min(DC.SIZES_FP16, key=lambda s: s[0] * s[1] * s[2] ** 2)
    for p in (0, 2):
        c["dct %dx%d u%g p%d" % (W, H, u, p)] = _family(W, H, p, u, lambda p=p, W=W, H=H, u=u: v.Upscaler(W, H, u, p, 0.2, 0, v.FLAG_DCT), _named("dct:"),
                                                        lambda x, p=p, W=W, H=H, u=u: D.resample_planes(x, D.out_size(W, u), D.out_size(H, u)) / D.upsq(u, p == 2))
    W, H, u = min(DN.SIZES, key=lambda s: s[0] * s[1] * s[2] ** 2)
    c["down %dx%d u%g p0" % (W, H, u)] = _family(W, H, 0, u, lambda W=W, H=H, u=u: v.Upscaler(W, H, u, 0, 0.2, 0, v.FLAG_DOWNSCALE), _named("downscale: size-generic"),
                                                 lambda x, W=W, H=H, u=u: S.fft_down_planes(x, S.out_size(W, u), S.out_size(H, u)) / DN._scale(W, H, u, False))
    W, H, u = min(DN.SIZES_DCT, key=lambda s: s[0] * s[1] * s[2] ** 2)
    c["down dct %dx%d u%g p2" % (W, H, u)] = _family(W, H, 2, u, lambda W=W, H=H, u=u: v.Upscaler(W, H, u, 2, 0.2, 0, v.FLAG_DOWNSCALE | v.FLAG_DCT), _named("downscale: dct:"),
                                                     lambda x, W=W, H=H, u=u: S.dct_down_planes(x, S.out_size(W, u), S.out_size(H, u)) / DN._scale(W, H, u, True, True))
    W, H, uW, uH, origin, span, extra = min(VW.VIEWS, key=lambda s: s[2] * s[3])
    for p in (0, 2):
        c["view %dx%d->%dx%d p%d" % (W, H, uW, uH, p)] = _family(
            W, H, p, V.effective_factor(uW, uH, span), lambda p=p, a=(W, H, uW, uH, origin, span): v.Upscaler.view(*a, p, 0.2, 0, VW._flags(v, extra)), _named("view:"),
            lambda x, a=(uW, uH, origin, span): V.view_planes(x, *a) / (a[0] * a[1] / (a[3][0] * a[3][1])))
    W, H, u = min(A.UP, key=lambda s: s[0] * s[1] * s[2] ** 2)
    c["any %dx%d u%g p0" % (W, H, u)] = _family(W, H, 0, u, lambda W=W, H=H, u=u: v.Upscaler(W, H, u, 0, 0.2, 0, v.FLAG_ANY_SIZE), _named("size-generic kernels (", "bluestein L="),
                                                lambda x, u=u: RL.closed_form(x, u))
    return c


IDS = ["generic 64x32 p0", "generic 64x32 p2", "generic 20x12 p1", "aot 512x256 p0", "aot 512x256 p2", "aot 1024x512 p0", "aot 2048x1024 p0", "aot 2048x1024 p2",
       "jit 128x64 p0", "jit 128x64 p2", "jit 640x480 p0", "jit 640x480 p2", "jit 486x294 p0", "jit 720x576 p0", "jit 640x480 u3 p0",
       "jit 1280x720 u1.5 p0"] \
    + ["%s pairs=%d" % (s, n) for n in (1, 2, 3) for s in ("aot 512x256 p0", "aot 512x256 p2", "jit 640x480 p0")] \
    + ["jit 640x480 p0 pairs=1439", "jit 640x480 p0 ring=3", "non-R2C 4608x16 p0", "four-step 9216x8 p0", "exact 50x32->50x35 p0 (odd uH)",
       "exact 50x32->63x32 p0 (odd uW)", "exact 50x32->63x35 p2 (odd both)", "odd 45x21 u2 p0", "dct 64x32 u2 p0", "dct 64x32 u2 p2", "down 16x512 u0.5 p0",
       "down dct 96x60 u0.5 p2", "view 50x32->32x20 p0", "view 50x32->32x20 p2", "any 46x22 u2 p0"]


@functools.lru_cache(maxsize=None)
def _all_cases():
    c = _cases()
    assert sorted(c) == sorted(IDS), sorted(set(c) ^ set(IDS))
    return c


@functools.lru_cache(maxsize=None)
def _run_case(name):
    """every frame of one case at the per-case bars; returns the -p 2 counts (differing R, R values, differing output, output values)
    of the last two rows of R and the last output row, for the pooled fraction bars"""
    case, (W, H) = _all_cases()[name]
    p, counts = case.precision, []
    with _knobs(case.knobs), case.make() as up:
        case.reaches(up)
        assert not up.u8_store
        if case.pairs is not None:
            want = case.pairs(up) if callable(case.pairs) else case.pairs
            assert want is not None and abs(_pairs_per_strip(up) - want) < 1e-6 * want, (name, _pairs_per_strip(up), want)
        for kind in case.kinds:
            tag = "last_row %s %s" % (name, kind)
            rgb = _kind_frame(kind, W, H, SEED[kind])
            up.upload_rgb8(rgb)
            up.execute(1)
            pre = up.download_presharpen()
            out = up.download_planar()[:, -3:].astype(np.float64)
            u8 = up.download_rgb8()[-3:]
            bar, l2_bar, own_bar, codes = _bars(p, kind, case.bit_exact)
            if kind in case.oracle_kinds:
                opre, oout, ou8 = case.oracle(kind)
                assert pre.shape == opre.shape
                pre = pre.astype(np.float64)
                if p == 2:
                    assert within_one_half_ulp(pre, opre).all(), tag
                    counts.append((int((pre[:, -2:] != opre[:, -2:]).sum()), pre[:, -2:].size, int((out[:, 2] != oout[:, 2]).sum()), out[:, 2].size))
                _rows(tag + " vs oracle", out, oout, bar, l2_bar)
                _codes(tag + " u8 vs oracle", u8, ou8, codes)
            elif p == 2 and kind in case.pre_kinds:
                opre = case.pre_oracle(kind)
                pre64 = pre.astype(np.float64)
                assert within_one_half_ulp(pre64, opre).all(), tag
                counts.append((int((pre64[:, -2:] != opre[:, -2:]).sum()), pre64[:, -2:].size, 0, 0))
            # the sharpen alone: rows uH-3 .. uH-1 from rows uH-4 .. uH-1 of the device's own pre-sharpen image
            if not case.own:
                continue
            own = O.sharpen(pre[:, -4:].astype(np.float64), case.u_e, p, 0.2)[:, 1:]
            _rows(tag + " vs sharpen(device's own pre-sharpen rows)", out, own, own_bar, l2_bar if case.two_launch else None)
            if kind not in case.oracle_kinds:
                _codes(tag + " u8 vs sharpen(own rows)", u8, _store_u8(own).transpose(1, 2, 0), codes)
    return tuple(counts)


@pytest.mark.parametrize("name", IDS)
def test_last_row(name):
    _run_case(name)


def test_pooled_fp16_fractions():
    """the two fraction bars of -p 2 (<= 1 % of R, <= 2 % of the output differ from the oracle's binary16 values) on the last rows of all
    -p 2 cases together (a case that already ran is not run again)"""
    acc = [t for name in IDS if _all_cases()[name][0].precision == 2 for t in _run_case(name)]
    assert len(acc) >= 10
    dp, npre, do, nout = (sum(col) for col in zip(*acc))
    measured("last_row pooled p2 (%d frames)" % len(acc), pre_diff_frac=dp / npre, out_diff_frac=do / nout, pre_values=npre, out_values=nout)
    assert dp <= 0.01 * npre
    assert do <= 0.02 * nout


@pytest.mark.parametrize("W,H,precision,full", [(512, 256, 0, True), (512, 256, 2, True), (2048, 1024, 0, False), (2048, 1024, 2, False)])
def test_fused_u8_store_last_row(W, H, precision, full):
    """FFTUP_FLAG_FUSE_U8_STORE: the fused kernel writes the interleaved 8-bit image itself, strips cut per plane.  Its last rows
    against the planes plan's 8-bit image (one code, test_fused_u8_store_equals_planes_plus_conversion) and against the oracle (one
    code, two at -p 2); at 2048x1024 the reference is the sharpen of the planes plan's own pre-sharpen rows."""
    import vkresample_amd as v
    for kind in ("NUEG" if full else "UG"):
        rgb = _kind_frame(kind, W, H, SEED[kind])
        with v.Upscaler(W, H, 2.0, precision) as up:
            _aot(up)
            up.upload_rgb8(rgb)
            up.execute(1)
            planes_u8 = up.download_rgb8()[-3:]
            pre = up.download_presharpen()[:, -4:].astype(np.float64)
        with v.Upscaler(W, H, 2.0, precision, 0.2, 0, v.FLAG_FUSE_U8_STORE) as up:
            _aot(up)
            assert up.u8_store and "8-bit RGB store" in up.description
            up.upload_rgb8(rgb)
            up.execute(1)
            got = up.download_rgb8()[-3:]
        tag = "last_row u8 store %dx%d p%d %s" % (W, H, precision, kind)
        _codes(tag + " vs planes + conversion", got, planes_u8, 1)
        ref = _fft_oracle(W, H, 2.0, precision, kind)[2] if full else _store_u8(O.sharpen(pre, 2.0, precision, 0.2)[:, 1:]).transpose(1, 2, 0)
        _codes(tag + (" vs oracle" if full else " vs sharpen(own rows)"), got, ref, 1 if precision == 0 else 2)


@pytest.mark.parametrize("W,H,precision,flags,reaches", [(512, 256, 0, 0, _aot), (512, 256, 2, 0, _aot), (128, 64, 0, 0, _jit("8*4*8 x128")), (60, 36, 0, 0, _generic)],
                         ids=["aot 512x256 p0", "aot 512x256 p2", "jit 128x64 p0", "generic 60x36 p0"])
def test_output_does_not_depend_on_the_previous_frame(W, H, precision, flags, reaches):
    """What an oracle comparison could miss on a lucky input: a tap of the bottom edge that reads memory the previous frame left (rows
    kept in LDS or registers, the padding behind a plane, another slot).  A uniform-noise frame, then frame B, on one plan: B's
    whole output and its pre-sharpen image are bit for bit those of B on a fresh plan -- with ring = 1 and with three slots, on
    planes and (fused plans) on the fused 8-bit store."""
    import vkresample_amd as v
    noise, B = _kind_frame("U", W, H, 950), _kind_frame("G", W, H, 951)
    fused = reaches is not _generic
    for ring in (1, 3):
        for store in ((False, True) if fused else (False,)):
            def run(frames):
                with v.Upscaler(W, H, 2.0, precision, 0.2, 0, flags | (v.FLAG_FUSE_U8_STORE if store else 0), ring) as up:
                    reaches(up)
                    assert up.u8_store == store
                    for f in frames:
                        for s in range(ring):
                            up.upload_rgb8(f, slot=s)
                        if ring == 1:
                            up.execute(1)
                        else:
                            up.execute_ring(ring, 0)
                    outs = [(up.download_rgb8(s) if store else up.download_planar(s)).copy() for s in range(ring)]
                    return outs, (None if store else up.download_presharpen().copy())
            fresh, fresh_pre = run([B])
            after, after_pre = run([noise, B])
            for s in range(ring):
                same = fresh[s] == after[s]
                rows = np.unique(np.argwhere(~same)[:, 0 if store else 1])
                assert same.all(), "ring %d store %d slot %d: %d values differ after a noise frame, rows %s" % (ring, store, s, int((~same).sum()), rows[:8])
                assert np.array_equal(fresh[s], fresh[0])
            if not store:
                assert np.array_equal(fresh_pre, after_pre)


def test_png_last_scanline():
    """the encoder's path: the last scanline of fftup_submit_png's file is fftup_submit_rgb8's last row, and both are the oracle's"""
    from PIL import Image
    import vkresample_amd as v
    W, H = 60, 36
    rgb = _kind_frame("G", W, H, 960)
    with v.Upscaler(W, H, 2.0, 0, 0.2, 0, 0, 1) as up:
        _generic(up)
        out = np.empty((2 * H, 2 * W, 3), np.uint8)
        up.wait(up.submit_rgb8(rgb, out))
        with v.PinnedArray((up.png_bound(),)) as buf:
            n = up.wait_png(up.submit_png(rgb), buf.array)
            img = np.asarray(Image.open(io.BytesIO(bytes(buf.array[:n]))).convert("RGB"))
    assert img.shape == out.shape and np.array_equal(img[-1], out[-1]) and np.array_equal(img, out)
    _codes("last_row png 60x36 vs oracle", img[-3:], O.upscale_rgb8(rgb, 2.0, 0, 0.2)[2][-3:], 1)
