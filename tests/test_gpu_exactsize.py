"""GPU: fftup_plan_create_size (Upscaler.to_size) -- an exact output size, one factor per axis, optional alignment of the pixel
centres -- against the fp64 statement of the rule, tests/exactsize_oracle.py, followed by oraclelib.sharpen with the effective
factor u_e = (float)sqrt(uW uH / (W H)) (quirks B4, B5; B1-B3 do not apply to these plans), at the bars of tests/paritylib.py.  The
amplitude-preserving image is sc * R, sc = uW uH / (W H).

The small cases are chosen so that each branch of the bin map is the only thing that can go wrong; each runs at both alignments,
-p 0 and -p 2, planar and fused-uint8 input.  One workload-sized case runs in the default run (1366x768 -> 1920x1080, -p 0, centres);
FFTUP_BIG_TESTS=1 adds -p 2."""
import os
import subprocess

import numpy as np
import pytest

import exactsize_oracle as E
import oraclelib as O
import paritylib as P
from paritylib import CLI

pytestmark = pytest.mark.gpu
BIG = os.environ.get("FFTUP_BIG_TESTS", "0") != "0"

# 50x32 -> 32x50: all even, rows folded, columns split (the mixed case); 40x30 -> 25x48: odd output row length, mixed; 64x48 -> 64x72:
# rows M = N; 45x21 -> 64x21: odd in, columns M = N with a tail row; 46x22 -> 70x30: Bluestein rows on both sides; 36x20: the identity
SMALL = [(50, 32, 32, 50, ""), (40, 30, 25, 48, ""), (64, 48, 64, 72, ""), (45, 21, 64, 21, ""), (46, 22, 70, 30, "any"), (36, 20, 36, 20, "")]


def _flags(v, extra):
    return v.FLAG_ANY_SIZE if "any" in extra else 0


def _run(W, H, uW, uH, precision, flags, align, rgb=None, planes=None):
    import vkresample_amd as v
    with v.Upscaler.to_size(W, H, uW, uH, precision, P.SHARPEN, 0, flags, align=align) as up:
        pre, out = P.run_uploaded(up, rgb, planes)
        names, desc = up.kernel_names, up.description
        assert (up.out_width, up.out_height) == (uW, uH)
        assert not up.tuned and not up.u8_store and up.num_kernels == 4
    return pre, out, names, desc


def _check(W, H, uW, uH, precision, extra, align, uint8, seed, tag, pooled=None):
    import vkresample_amd as v
    rgb, planes, x = P.inputs(W, H, precision, uint8, seed)
    pre, out, names, desc = _run(W, H, uW, uH, precision, _flags(v, extra) | (v.FLAG_FUSE_U8_LOAD if uint8 else 0), align, rgb, planes)
    assert all("_odd" in n for n in names[:3]) and names[3] == "sharpen", names
    assert "rows %d->%d" % (W, uW) in desc and "columns %d->%d" % (H, uH) in desc, desc
    assert ("centres" in desc) == (align == E.ALIGN_CENTRE), desc
    R = E.resample_R(x, uW, uH, align)
    sc = uW * uH / (W * H)
    u_e = E.effective_factor(W, H, uW, uH)
    assert pre.shape == R.shape == (3, uH, uW)
    P.assert_parity(tag, precision, pre, out, sc * R, sc, u_e, pooled=pooled)
    return pre, x


@pytest.mark.parametrize("uint8", [False, True])
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("align", [E.ALIGN_CORNER, E.ALIGN_CENTRE])
@pytest.mark.parametrize("W,H,uW,uH,extra", SMALL)
def test_exactsize_parity(W, H, uW, uH, extra, align, precision, uint8):
    pre, x = _check(W, H, uW, uH, precision, extra, align, uint8, W + H + uW + precision,
                    "exactsize p%d %dx%d->%dx%d a%d %s u8%d" % (precision, W, H, uW, uH, align, extra, uint8))
    if (W, H) == (uW, uH) and precision == 0:
        # the identity at both alignments (the oracle reproduces the input to 1e-15)
        P.assert_identity("exactsize identity %dx%d a%d" % (W, H, align), pre, x)


@pytest.mark.parametrize("precision", [0, 2] if BIG else [0])
def test_exactsize_parity_1366x768_to_1080p(precision):
    _check(1366, 768, 1920, 1080, precision, "any", E.ALIGN_CENTRE, False, 11, "exactsize p%d 1366x768->1920x1080 centres" % precision)


@pytest.mark.parametrize("W,H,uW,uH,extra", [(46, 22, 70, 30, "any"), (50, 32, 32, 50, "")])
def test_cosine_comes_back_at_the_centre_aligned_positions(W, H, uW, uH, extra):
    """what the oracle alone cannot hide: rows 0.5 + a cos(2 pi k x / W + 0.4) come back as the same cosine at x = (m + 1/2) W / uW - 1/2,
    for k = 1 and the largest k below min(W, uW)/2 (a bin that is copied, not split or folded)"""
    import vkresample_amd as v
    a, sc = 0.3, uW * uH / (W * H)
    pos = (np.arange(uW) + 0.5) * W / uW - 0.5
    for k in (1, (min(W, uW) - 1) // 2):
        row = 0.5 + a * np.cos(2 * np.pi * k * np.arange(W) / W + 0.4)
        x = np.ascontiguousarray(np.broadcast_to(row, (3, H, W)).astype(np.float32))
        pre, _, _, _ = _run(W, H, uW, uH, 0, _flags(v, extra), E.ALIGN_CENTRE, planes=x)
        want = np.broadcast_to(0.5 + a * np.cos(2 * np.pi * k * pos / W + 0.4), (3, uH, uW))
        P.measured("exactsize cosine %d->%d k=%d" % (W, uW, k), max_err=np.abs(sc * pre - want).max(), l2=P.rel_l2(sc * pre, want))
        assert P.rel_l2(sc * pre, want) <= P.FP32_PRE_L2
        assert np.abs(sc * pre - want).max() <= P.FP32_PRE_MAX


@pytest.mark.parametrize("W,H,uW,uH,extra", [(46, 22, 70, 30, "any"), (50, 32, 32, 50, ""), (40, 30, 25, 48, "")])
def test_mirroring_the_input_mirrors_the_output(W, H, uW, uH, extra):
    """centre alignment commutes with mirroring both axes (corner alignment does not: tests/test_exactsize_oracle.py); compared on
    the pre-sharpen image, whose sharpen pass has a direction of its own (quirk B5)"""
    import vkresample_amd as v
    _, planes, _ = P.inputs(W, H, 0, False, 21)
    sc = uW * uH / (W * H)
    a, _, _, _ = _run(W, H, uW, uH, 0, _flags(v, extra), E.ALIGN_CENTRE, planes=np.ascontiguousarray(planes[:, ::-1, ::-1]))
    b, _, _, _ = _run(W, H, uW, uH, 0, _flags(v, extra), E.ALIGN_CENTRE, planes=planes)
    b = b[:, ::-1, ::-1]
    P.measured("exactsize mirror %dx%d->%dx%d" % (W, H, uW, uH), max_err=sc * np.abs(a - b).max(), l2=P.rel_l2(a, b))
    assert P.rel_l2(a, b) <= P.FP32_PRE_L2 and sc * np.abs(a - b).max() <= P.FP32_PRE_MAX


@pytest.mark.parametrize("precision", [0, 2])
def test_corner_aligned_u2_is_the_oddsize_plan(precision):
    """1215x675 -> 2430x1350, corners: u_e = 2 exactly, the same kernels without a phase table -- the bytes of FLAG_ODD_SIZE -u 2"""
    import vkresample_amd as v
    rgb = P.frame(1215, 675, seed=31)
    got = []
    for make in (lambda: v.Upscaler(1215, 675, 2.0, precision, 0.2, 0, v.FLAG_ODD_SIZE),
                 lambda: v.Upscaler.to_size(1215, 675, 2430, 1350, precision, 0.2, 0, 0, align=E.ALIGN_CORNER)):
        with make() as up:
            up.upload_rgb8(rgb)
            up.execute(1)
            got.append((up.download_planar().tobytes(), up.output_checksum(), up.kernel_names, up.alg_bytes_per_frame, up.kernel_alg_bytes,
                        up.kernel_min_bytes))
    assert got[0][1:] == got[1][1:]
    assert got[0][0] == got[1][0]
    assert got[0][1] == P.word_sum(got[0][0])


def test_existing_plans_keep_their_results():
    """one FLAG_ODD_SIZE plan and one plain even plan (size-generic kernels) against the oracle bars they already meet: the phase
    tables are null for them"""
    import vkresample_amd as v
    from test_gpu_oddsize import _check as odd_check
    odd_check(45, 21, 2.0, 0, "", False, 66, "oddsize p0 45x21 u2 (beside exact-size plans)")
    odd_check(125, 75, 0.6, 2, "down", True, 202, "oddsize p2 125x75 u0.6 down (beside exact-size plans)")
    rgb = P.frame(240, 126, seed=7)
    with v.Upscaler(240, 126, 2.0, 0, 0.2, 0, v.FLAG_GENERIC_KERNELS) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        pre = up.download_presharpen().astype(np.float64)
        out = up.download_planar().astype(np.float64)
        assert up.kernel_names == ["row_r2c", "col_fwd_pad_inv", "row_c2r", "sharpen"] and "exact" not in up.description
    opre, oout, _ = O.upscale_rgb8(rgb, 2.0, 0, 0.2)
    P.measured("even plan 240x126 u2", pre_l2=P.rel_l2(pre, opre), pre_max=4 * np.abs(pre - opre).max(), out_l2=P.rel_l2(out, oout),
               out_max=np.abs(out - oout).max())
    assert P.rel_l2(pre, opre) <= P.FP32_PRE_L2 and 4 * np.abs(pre - opre).max() <= P.FP32_PRE_MAX
    assert P.rel_l2(out, oout) <= P.FP32_OUT_L2 and np.abs(out - oout).max() <= P.FP32_OUT_MAX


@pytest.mark.parametrize("precision", [0, 2])
def test_every_execution_path_gives_the_same_bytes(precision):
    """50x32 -> 32x50, centres, ring 3: execute against execute_ring slot by slot, submit_rgb8 and submit_png against upload + execute +
    download_rgb8, FLAG_OVERLAP_ITERATIONS against ordered iterations, the checksum equal to the sum of the words"""
    import vkresample_amd as v
    W, H, uW, uH, al = 50, 32, 32, 50, E.ALIGN_CENTRE
    frames = [np.ascontiguousarray(P.frame(W, H, seed=60 + k)) for k in range(3)]
    want, planes, sums = [], [], []
    with v.Upscaler.to_size(W, H, uW, uH, precision, 0.2, 0, 0, align=al) as up:
        for f in frames:
            up.upload_rgb8(f)
            up.execute(1)
            want.append(up.download_rgb8())
            planes.append(up.download_planar().tobytes())
            sums.append(up.output_checksum())
            assert sums[-1] == P.word_sum(planes[-1])
        ms = up.profile_kernels(2)
        assert len(ms) >= 4 and all(t > 0 for t in list(ms)[:4])
    with v.Upscaler.to_size(W, H, uW, uH, precision, 0.2, 0, v.FLAG_OVERLAP_ITERATIONS, align=al) as up:
        up.upload_rgb8(frames[0])
        up.execute(5)
        assert up.download_planar().tobytes() == planes[0]
        assert up.output_checksum() == sums[0]
    more = v.FLAG_FUSE_U8_STORE | v.FLAG_TUNE_PLAN | v.FLAG_UNFUSED_SHARPEN | v.FLAG_GENERIC_KERNELS | v.FLAG_ODD_SIZE | v.FLAG_DOWNSCALE
    with v.Upscaler.to_size(W, H, uW, uH, precision, 0.2, 0, more, 3, align=al) as up:
        assert not up.u8_store and not up.tuned and up.num_kernels == 4
        for s, f in enumerate(frames):
            up.upload_rgb8(f, s)
        up.execute_ring(3)
        for s in range(3):
            assert up.download_planar(s).tobytes() == planes[s], s
            assert np.array_equal(up.download_rgb8(s), want[s]), s
            assert up.output_checksum(s) == sums[s], s
        up.execute_ring_timed(3)
        assert up.download_planar(1).tobytes() == planes[1]
        out = np.empty((uH, uW, 3), np.uint8)
        for k in (1, 2, 0):
            up.wait(up.submit_rgb8(frames[k], out))
            assert np.array_equal(out, want[k]), k
        buf = np.empty(up.png_bound(), np.uint8)
        for k in (2, 0):
            n = up.wait_png(up.submit_png(frames[k]), buf)
            assert np.array_equal(P.png_pixels(bytes(buf[:n]), uW, uH), want[k]), k


def test_plan_info_and_errors():
    import vkresample_amd as v
    from test_host_exactsize import INVALID
    with v.Upscaler.to_size(50, 32, 32, 50, align=E.ALIGN_CENTRE) as up:
        assert up.kernel_names == ["row_r2c_crop_odd", "col_fwd_pad_inv_odd", "row_c2r_odd", "sharpen"]
        assert up.num_kernels == 4 and not up.tuned and not up.u8_store
        assert "rows 50->32" in up.description and "columns 32->50" in up.description and "centres" in up.description
        assert "bluestein" not in up.description
    with v.Upscaler.to_size(50, 32, 32, 50) as up:
        assert "rows 50->32" in up.description and "columns 32->50" in up.description and "centres" not in up.description
    with v.Upscaler.to_size(1366, 768, 1920, 1080, 2, flags=v.FLAG_ANY_SIZE, align=E.ALIGN_CENTRE) as up:
        assert up.kernel_names == ["row_r2c_odd_bz", "col_fwd_pad_inv_odd", "row_c2r_odd", "sharpen"]
        assert "rows 1366->1920 bluestein" in up.description and "centres" in up.description
    # sizes with ahead-of-time or plan-time kernels under fftup_plan_create stay on the four size-generic launches here
    for (W, H, uW, uH) in [(512, 256, 1024, 512), (1920, 1080, 3840, 2160), (640, 480, 960, 720)]:
        with v.Upscaler.to_size(W, H, uW, uH) as up:
            assert up.kernel_names == ["row_r2c_odd", "col_fwd_pad_inv_odd", "row_c2r_odd", "sharpen"] and not up.tuned and up.num_kernels == 4
    # the same codes as without a device (tests/test_host_exactsize.py)
    for kwargs, code, word in INVALID:
        with pytest.raises(v.FftupError) as e:
            v.Upscaler.to_size(**kwargs)
        assert e.value.code == code and word in str(e.value), (kwargs, str(e.value))


def test_exactsize_cli(tmp_path):
    """-size 70x30 -centres -anysize on a 46x22 PNG gives the API's pixels, single-image and batched (host and -gpupng encoders); -size
    with -u and -centres without -size exit 1 with a message and write nothing"""
    import vkresample_amd as v
    rgb = P.frame(46, 22, seed=78)
    with v.Upscaler.to_size(46, 22, 70, 30, 0, 0.2, 0, v.FLAG_ANY_SIZE, align=E.ALIGN_CENTRE) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        want = up.download_rgb8()
    with v.Upscaler.to_size(46, 22, 70, 30, 0, 0.2, 0, v.FLAG_ANY_SIZE, align=E.ALIGN_CORNER) as up:
        up.upload_rgb8(rgb)
        up.execute(1)
        corner = up.download_rgb8()
    assert not np.array_equal(want, corner)
    P.png_write(tmp_path / "in.png", rgb)

    def cli(*args):
        return subprocess.run([CLI] + list(args), capture_output=True, text=True, cwd=tmp_path, timeout=120)

    r = cli("-i", "in.png", "-o", "out.png", "-size", "70x30", "-centres", "-anysize", "-n", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "46x22 to 70x30" in r.stdout
    assert np.array_equal(P.png_read(tmp_path / "out.png"), want)
    r = cli("-i", "in.png", "-o", "corner.png", "-size", "70x30", "-anysize")
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(P.png_read(tmp_path / "corner.png"), corner)
    r = cli("-i", "in.png", "-o", "bad.png", "-size", "70x30", "-u", "2", "-anysize")
    assert r.returncode == 1 and "-u" in r.stdout and not (tmp_path / "bad.png").exists()
    r = cli("-i", "in.png", "-o", "bad.png", "-u", "2", "-centres", "-anysize")
    assert r.returncode == 1 and "-size" in r.stdout and not (tmp_path / "bad.png").exists()
    r = cli("-i", "in.png", "-o", "bad.png", "-size", "70", "-anysize")
    assert r.returncode == 1 and not (tmp_path / "bad.png").exists()
    (tmp_path / "inp").mkdir()
    for k, extra in enumerate(([], ["-gpupng"])):
        outp = tmp_path / ("outp%d" % k)
        outp.mkdir()
        for n in (1, 2):
            P.png_write(tmp_path / "inp" / ("%06d.png" % n), rgb)
        r = cli("-ifolder", "inp", "-ofolder", outp.name, "-numfiles", "2", "-size", "70x30", "-centres", "-anysize", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        for n in (1, 2):
            assert np.array_equal(P.png_read(outp / ("%06d.png" % n)), want), (extra, n)
