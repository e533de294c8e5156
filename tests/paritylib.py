"""The parity bars of the plan families and the helpers their GPU tests share.  Test infrastructure only: no test lives here,
and vkresample_amd is imported only by the functions that need a device.

The bars (north_star: "within 1e-4 rel-err").  Every bound is about ten times the largest figure any parametrisation measured
(printed as MEASURED lines under pytest -s: profiles/r04_h_parity_small.txt, profiles/family_sweep_long.txt), so it is the error
budget of THIS code and not of the task.  A family's oracle states the amplitude-preserving image y; the plan stores R = y / sc
(sc: u^2, uW uH / (W H), ... -- the family module says which) and sharpens R.
  fp32 (-p 0): sc * pre within relative L2 FP32_PRE_L2 and max FP32_PRE_MAX (of full scale) of y; the sharpened output within
      relative L2 FP32_OUT_L2 and max FP32_OUT_MAX of oraclelib.sharpen applied to the oracle's R.  These are the bars of
      natural-like frames: the reference's filter has scale = -s*sqrt(min(a,b)), whose slope is unbounded at 0, and the allowances
      for uniform noise that follow from it are tests/test_gpu_parity.py's own.
  fp16 (-p 2): the plan stores binary16 (half ulp 2.4e-4 at 0.5).  R within one binary16 ulp of the oracle's own binary16 value
      -- fp32-vs-fp64 transform noise can flip a rounding -- and different from it in at most FP16_PRE_DIFF_FRAC of the values
      (ringing around zero: the ulp shrinks with |R|, the fp32 noise does not); the sharpened output, against oraclelib.sharpen of
      the oracle's binary16 R, within relative L2 FP16_OUT_L2, different in at most FP16_OUT_DIFF_FRAC of the values, max
      FP16_OUT_MAX = 16 ulps (errors come in whole ulps; a one-ulp flip of an input moves the binary16-arithmetic filter by a few).
The last output row is compared like every other: the reference reads stale padding memory there (quirk B5), this project defines
those reads as "same column, last written row" (oracle/fftup_oracle.c) and every comparison holds the HIP path to that definition.
"""
import os
import struct
import zlib

import numpy as np

import oraclelib as O
from family_sweep_cases import smooth  # noqa: F401  (the one definition: 2, 3, 5, 7-smooth, False below 1)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vkresample_amd", "vkresample")

SHARPEN = 0.2                  # the strength every family plan is opened with
FP32_PRE_L2 = 2e-6             # (measured <= 3.5e-7)
FP32_PRE_MAX = 1e-5            # (<= 9.5e-7)
FP32_OUT_L2 = 5e-6             # (<= 7.7e-7)
FP32_OUT_MAX = 2e-5            # (<= 2.7e-6)
HALF_ULP_SLACK = 1.0001        # one ulp, and the rounding of the comparison itself
HALF_ULP_FLOOR = 5e-7          # below |R| ~ 2^-14 the binary16 grid (2^-24) is finer than the fp32 transform's own noise
FP16_PRE_DIFF_FRAC = 0.01      # (<= 0.87 %)
FP16_OUT_L2 = 3.5e-4           # (<= 2.2e-4)
FP16_OUT_MAX = 8e-3            # (<= 2.9e-3)
FP16_OUT_DIFF_FRAC = 0.02      # (<= 1.98 %: 48x30 -> 48x48, exact ties; 0.23 % elsewhere)


# ------------------------------------------------------------------------------------------------------------------- primitives
def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30))


def measured(tag, **vals):
    """the error figures of a comparison, printed (pytest -s -> profiles/): the asserted bounds sit at about ten times the largest
    figure any parametrisation printed"""
    print("MEASURED %s: %s" % (tag, "  ".join("%s %.3g" % kv for kv in vals.items())))


def frame(W, H, seed=0, dist="N"):
    from vkresample_amd import synth
    return synth.frame(seed, W, H, dist)


def half_ulp(opre):
    """one binary16 ulp at each value of `opre` (normal numbers: 2^-10 |x| bounds it from above)"""
    return np.maximum(np.abs(opre), 2.0 ** -14) * 2.0 ** -10


def one_half_ulp_bound(opre):
    return half_ulp(opre) * HALF_ULP_SLACK + HALF_ULP_FLOOR


def within_one_half_ulp(pre, opre):
    """per value: `pre` is a binary16 neighbour of `opre`, or `opre` itself"""
    return np.abs(pre - opre) <= one_half_ulp_bound(opre)


# --------------------------------------------------------------------------------------------------------------- inputs and run
def inputs(W, H, precision, uint8, seed):
    """(rgb, planes, x): what is uploaded and the values the plan computes on.  Planar input: a natural-like frame as floats
    (x / 255 plus a little noise below one 8-bit step), in the plan's storage type -- the bars are those of natural frames"""
    rgb = frame(W, H, seed=seed)
    if uint8:
        return rgb, None, O.load_lut(precision)[np.transpose(rgb, (2, 0, 1))]
    x = np.transpose(rgb, (2, 0, 1)) / 255.0 + np.random.RandomState(seed).rand(3, H, W) / 512.0
    planes = x.astype(np.float16 if precision == 2 else np.float32)
    return None, planes, planes.astype(np.float64)


def run_uploaded(up, rgb=None, planes=None):
    """upload whichever is given, one frame -> (pre-sharpen image, output) as float64"""
    if rgb is not None:
        up.upload_rgb8(rgb)
    else:
        up.upload_planar(planes)
    up.execute(1)
    return up.download_presharpen().astype(np.float64), up.download_planar().astype(np.float64)


# --------------------------------------------------------------------------------------------------------------- the comparison
def assert_parity(tag, precision, pre, out, y, sc, u, pooled=None):
    """one frame of a plan against its family's oracle at the bars above.  `y`: the oracle's amplitude-preserving image, R = y / sc
    what the plan stores, `u` the factor of the sharpen pass; `pre` None: the output alone.  `pooled`: a list that takes the -p 2
    counts (differing R, all R, differing output, all output) in place of the two fraction bars -- an output of a few dozen
    values, whose fractions pooled_fraction_bars asserts over all such cases together"""
    assert precision in (0, 2)
    R = y / sc
    out = np.asarray(out, np.float64)
    figs = {}
    if precision == 0:
        sh = O.sharpen(R, u, 0, SHARPEN)
        if pre is not None:
            figs.update(pre_l2=rel_l2(sc * pre, y), pre_max=np.abs(sc * pre - y).max())
        figs.update(out_l2=rel_l2(out, sh), out_max=np.abs(out - sh).max())
    else:
        opre = R.astype(np.float16).astype(np.float64)
        sh = O.sharpen(opre, u, 2, SHARPEN)
        if pre is not None:
            figs.update(pre_diff_frac=(pre != opre).mean(), pre_max_ulps=(np.abs(pre - opre) / half_ulp(opre)).max())
        figs.update(out_l2=rel_l2(out, sh), out_max=np.abs(out - sh).max(), out_diff_frac=(out != sh).mean())
    measured(tag, **figs, last_row_max=np.abs(out[:, -1] - sh[:, -1]).max())
    if precision == 0:
        if pre is not None:
            assert rel_l2(sc * pre, y) <= FP32_PRE_L2
            assert np.abs(sc * pre - y).max() <= FP32_PRE_MAX
        assert rel_l2(out, sh) <= FP32_OUT_L2
        assert np.abs(out - sh).max() <= FP32_OUT_MAX                   # (the last row included)
    else:
        if pre is not None:
            assert within_one_half_ulp(pre, opre).all()
        assert rel_l2(out, sh) <= FP16_OUT_L2
        assert np.abs(out - sh).max() <= FP16_OUT_MAX
        if pooled is None:
            assert pre is None or (pre != opre).mean() <= FP16_PRE_DIFF_FRAC
            assert (out != sh).mean() <= FP16_OUT_DIFF_FRAC
        else:
            counts = (0, 0) if pre is None else (int((pre != opre).sum()), pre.size)
            pooled.append(counts + (int((out != sh).sum()), out.size))


def assert_identity(tag, pre, x):
    """-u 1 / M = N: the plan reproduces its input (the oracles do, to 1e-15) at the fp32 pre-sharpen bars"""
    measured(tag, max_err=np.abs(pre - x).max(), l2=rel_l2(pre, x))
    assert rel_l2(pre, x) <= FP32_PRE_L2 and np.abs(pre - x).max() <= FP32_PRE_MAX


def pooled_fraction_bars(tag, acc):
    """the two -p 2 fraction bars on the counts assert_parity appended to `acc`, all cases together"""
    dp, npre, do, nout = (sum(col) for col in zip(*acc))
    measured(tag, pre_diff_frac=dp / npre, out_diff_frac=do / nout, pre_values=npre, out_values=nout)
    assert dp <= FP16_PRE_DIFF_FRAC * npre
    assert do <= FP16_OUT_DIFF_FRAC * nout


def word_sum(b):
    """fftup_output_checksum in numpy: the 32-bit little-endian words, the bytes behind the last whole word as one more"""
    b = b + b"\0" * (-len(b) % 4)
    return int(np.frombuffer(b, "<u4").astype(np.uint64).sum() & np.uint64(0xFFFFFFFFFFFFFFFF))


# --------------------------------------------------------------------------------------------------------------------------- PNG
def png_write(path, rgb):
    from PIL import Image
    Image.fromarray(rgb).save(path)


def png_read(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def png_pixels(png, uW, uH):
    """the RGB image of a PNG file of 8-bit RGB (zlib + the five row filters)"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat = 8, b""
    while pos < len(png):
        n, = struct.unpack(">I", png[pos:pos + 4])
        if png[pos + 4:pos + 8] == b"IDAT":
            idat += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    raw = zlib.decompress(idat)
    stride = 3 * uW
    assert len(raw) == uH * (stride + 1)
    img = np.zeros((uH, stride), np.int64)
    prev = np.zeros(stride, np.int64)
    for r in range(uH):
        ft = raw[r * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, r * (stride + 1) + 1).astype(np.int64)
        cur = np.zeros(stride, np.int64)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        else:
            for i in range(stride):
                a = cur[i - 3] if i >= 3 else 0
                b = prev[i]
                c = prev[i - 3] if i >= 3 else 0
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (line[i] + p) & 255
        img[r] = cur
        prev = cur
    return img.reshape(uH, uW, 3).astype(np.uint8)
