"""Run-time specialised plans (csrc/jit.hpp): a size with an integer upscale factor and no ahead-of-time kernels gets its row, column and fused
C2R+sharpen kernels instantiated through hipRTC at plan time.  Parity against the oracle (same tolerances as
test_gpu_parity.test_full_size_vs_oracle) and against the size-generic kernels on the same frame, for sizes that
exercise every plan family: three-stage mixed-radix rows/columns, power-of-two rows/columns, the 16*16*R fused plans,
the N-stage fused plans (four stages, several butterflies per thread), the stand-alone C2R of the pre-sharpen tap."""

import numpy as np
import pytest

import oraclelib as O
from paritylib import rel_l2, within_one_half_ulp
from test_gpu_parity import _report, _run, _up

pytestmark = pytest.mark.gpu

# (W, H): row plan / column plan / fused plan as chosen by jit.hpp
JIT_SIZES = [
    (640, 480),     # 10*8*8 / 5*8*12 / 16*16*5
    (720, 576),     # 9*8*10 / 9*8*8 / 12*8*15 on 128 threads
    (1000, 1000),   # 10*10*10 (even first radix) / 10*10*10 / 8*5*5*10 (four stages)
    (1024, 768),    # power of two / 8*8*12 / FusedPlanPow2<2048>
    (1280, 1024),   # 10*8*16 / power of two / 16*16*10
    (1600, 900),    # 10*10*16 / 9*10*10 / 16*2*10*10: 5 butterflies of radix 2 per thread
    (896, 504),     # radix 7: 7*8*16 / 7*8*9 / 16*16*7
    (128, 64),      # smallest sizes that are specialised
    (1200, 512),    # 512 rows: the digit-swap column kernel on four waves (k_col_v<4, 512>)
    (960, 256),     # 256 rows: ... on two waves
    (2000, 1250),   # no three-stage factorization: N-stage row 8*5*5*10, column 5*5*5*10 on 1024 threads, fused 8*5*10*10
    (486, 294),     # 9*2*3*9 / 7*2*3*7 / 12*9*9
    (640, 3000),    # a column length whose first and last stage need 300 threads: two columns per workgroup (10*3*10*10)
    (1792, 1008),   # 7*16*16 / 7*12*12 / 8*7*8*8 on 512 threads (a quarter of 3584x2016, whose fused plan is 8*8*16*7 on 1024 threads)
    (3840, 2160),   # 4K -> 8K: 15*16*16 / 15*12*12 on 720 threads / 8*8*10*12 on 960 threads, 61 KB of LDS
]


@pytest.mark.parametrize("W,H", JIT_SIZES)
@pytest.mark.parametrize("precision,flags", [(0, 0), (0, 2), (2, 2)])
def test_specialised_plan_vs_oracle(W, H, precision, flags):
    with _up(W, H, 2.0, precision, 0.2, 0, flags) as up:
        assert up.tuned and up.specialised_at_plan_time, "plan fell back to the size-generic kernels"
    (pre, out, u8), (opre, oout, ou8) = _run(W, H, 2.0, precision, "N", flags=flags, seed=W + H)
    tag = "jit %dx%d p%d flags%d" % (W, H, precision, flags)
    if precision == 0:
        so = _report(tag + " out", out - oout, 1e-4)
        # (about ten times the measured distributions, profiles/r02_q_pytest_gpu.txt: max 1.2e-6 .. 2.1e-6, p99.99 1.2e-6)
        assert rel_l2(pre, opre) <= 2e-6 and np.abs(pre - opre).max() * 4 <= 1e-5
        assert so["p99.99"] <= 1.2e-5 and so["max"] <= 2e-5 and so["count_above"] == 0
        d = np.abs(u8.astype(int) - ou8.astype(int))
        assert d.max() <= 1 and (d != 0).mean() <= 5e-4
    else:
        assert within_one_half_ulp(pre, opre).all()
        so = _report(tag + " out", out - oout, 2.0 ** -10)
        assert so["max"] <= 8e-3 and so["p99"] == 0 and so["p99.99"] <= 3e-3 and so["count_above"] <= 5e-4 * so["n"]      # (measured: max <= 4.6e-3, p99.99 <= 1.5e-3, <= 1.5e-4 n)


# upscale factors other than 2.  Integer: U - 1 residue transforms in the column kernel (k_col_u), first radix of the fused
# kernel a multiple of 2U
U_CASES = [
    (640, 480, 3.0),     # fused 12*10*16
    (640, 480, 4.0),     # fused 16*16*10 (FusedPlanMr16, NI = 2)
    (1024, 512, 4.0),    # FusedPlanPow2<4096> with one non-zero input per first-stage butterfly
    (1280, 720, 3.0),    # fused 12*4*5*16
    (960, 540, 4.0),     # 540p -> 2160p
    (640, 480, 5.0),     # first radix 10
    (256, 128, 8.0),     # first radix 16, NI = 1
    (2048, 1024, 3.0),   # 6144 x 3072
    # half-integer factors: k_col_pad (forward H, zero-pad, inverse uH in one kernel), fused kernel with U = 1, D = 2u
    (1280, 720, 1.5),    # 720p -> 1080p: fused 12*10*16, one third of the first-stage inputs non-zero
    (1920, 1080, 1.5),
    (2560, 1440, 1.5),   # 1440p -> 4K
    (640, 480, 2.5),     # first radix 10, D = 5
    (1280, 2160, 1.5),   # uH = 3240: k_col_pad with two columns per workgroup
    (640, 3000, 3.0),    # k_col_u with two columns per workgroup
    (5120, 2880, 1.5),   # 5K -> 8K: the widest input (7680 output columns), uH = 4320
    # quarter-integer factors (round 5): the factor is D / (2 DD) with DD = 2 -- the fused kernel's first radix makes R0 DD / D whole
    (1280, 720, 1.25),   # 5/4: fused 10*10*16, NI = 4 of 10 first-stage inputs non-zero
    (1024, 512, 1.25),   # row pow2/8, fused 10*8*16
    (1920, 1080, 1.25),  # 1080p -> 2400 x 1350
    (1024, 768, 1.75),   # 7/4: first radix 7, NI = 2
    (1280, 720, 2.25),   # 9/4: first radix 9, NI = 4
    # an odd number of eighths (round 5, DD = 4): the two such factors whose numerator is a radix of the engine
    (1280, 720, 1.125),  # 9/8: 720p -> 1440 x 810, first radix 9, NI = 4 of 9 first-stage inputs non-zero
    (1024, 576, 1.875),  # 15/8: -> 1920 x 1080, first radix 15, NI = 4 of 15
    (2048, 1024, 1.125), # -> 2304 x 1152
    # ratios with denominator 3, 5, 7 (round 5, DD = 3, 5, 7): whatever float the caller passes, where the reference's float arithmetic
    # gives exact output sizes and the symmetric guard for THIS size (plan_rules.cpp: jit_factor)
    (1920, 1080, float(np.float32(4.0 / 3.0))),   # 1080p -> 1440p: fused 16*16*10, NI = 6 of 16 first-stage inputs non-zero
    (960, 540, float(np.float32(4.0 / 3.0))),     # -> 720p
    (1600, 900, 1.6),                             # 8/5: 900p -> 1440p
    (1000, 500, 1.4),                             # 7/5: first radix 14
    (1152, 648, float(np.float32(5.0 / 3.0))),    # 5/3: -> 1080p, first radix 10
    (1280, 720, 1.2),                             # 6/5: first radix 12
    (768, 432, float(np.float32(8.0 / 3.0))),     # 8/3
    (1120, 630, float(np.float32(8.0 / 7.0))),    # 8/7: -> 720p
    # ... and where that arithmetic puts the guard a row off the symmetric one (k_col_pad takes the guard as a parameter)
    (1600, 900, 1.2),                             # guard [449, 630) instead of [450, 630)
    (200, 100, 1.2),                              # [49, 70)
    (400, 270, 1.4),                              # [135, 242) instead of [135, 243): row 242 reads the UN-shifted F[242] (below H)
    (224, 98, float(np.float32(8.0 / 7.0))),      # [48, 63)
    (640, 480, 7.0),     # -u 7: first radix 14 = 2 x 7 (round 5), six residue transforms in the column kernel
    (320, 240, 7.0),
    (640, 480, 3.5),     # 7/2: first radix 14 as well
    # inputs taller than 4096 rows (round 5: up to 8192): two columns of a spectrum tile per workgroup (four no longer fit the LDS)
    (256, 8192, 2.0),    # col 16*2*16*16, 1024 threads
    (400, 6000, 2.0),
    (640, 4800, 3.0),    # k_col_u with two columns of 4800 points
]


@pytest.mark.parametrize("W,H,u", U_CASES)
@pytest.mark.parametrize("precision,flags", [(0, 0), (2, 2)])
def test_specialised_integer_factor_vs_oracle(W, H, u, precision, flags):
    with _up(W, H, u, precision, 0.2, 0, flags) as up:
        assert up.tuned and up.specialised_at_plan_time, "plan fell back to the size-generic kernels"
    (pre, out, u8), (opre, oout, ou8) = _run(W, H, u, precision, "N", flags=flags, seed=W + H)
    tag = "jit %dx%d u%g p%d flags%d" % (W, H, u, precision, flags)
    if precision == 0:
        so = _report(tag + " out", out - oout, 1e-4)
        assert rel_l2(pre, opre) <= 2e-6 and np.abs(pre - opre).max() * u * u <= 1e-5
        assert so["p99.99"] <= 1.2e-5 and so["max"] <= 2e-5 and so["count_above"] == 0
        d = np.abs(u8.astype(int) - ou8.astype(int))
        assert d.max() <= 1 and (d != 0).mean() <= 5e-4
    else:
        assert within_one_half_ulp(pre, opre).all()
        so = _report(tag + " out", out - oout, 2.0 ** -10)
        assert so["max"] <= 8e-3 and so["p99"] == 0 and so["p99.99"] <= 3e-3 and so["count_above"] <= 5e-4 * so["n"]      # (measured: max <= 4.6e-3, p99.99 <= 1.5e-3, <= 1.5e-4 n)


@pytest.mark.parametrize("W,H", [(640, 480), (1000, 1000), (1600, 900)])
def test_specialised_equals_generic(W, H):
    """same frame through the specialised plan and through the size-generic kernels (FFTUP_FLAG_GENERIC_KERNELS)"""
    from vkresample_amd import FLAG_GENERIC_KERNELS
    (pre, out, _), _ = _run(W, H, 2.0, 0, "U", seed=3)
    with _up(W, H, 2.0, 0, 0.2, 0, FLAG_GENERIC_KERNELS) as up:
        assert not up.tuned
    (pre2, out2, _), _ = _run(W, H, 2.0, 0, "U", seed=3, flags=FLAG_GENERIC_KERNELS)
    assert np.abs(pre - pre2).max() * 4 <= 4e-6
    assert np.percentile(np.abs(out - out2), 99.99) <= 1e-5


def test_specialisation_can_be_switched_off(monkeypatch):
    monkeypatch.setenv("FFTUP_JIT", "0")
    with _up(640, 480, 2.0, 0) as up:
        assert not up.tuned


def _knobs(monkeypatch, text):
    """FFTUP_EXPERIMENT is parsed by the test build of the library only (libfftup_knobs.so, -DFFTUP_TEST_KNOBS): load that one"""
    from vkresample_amd import _lib
    monkeypatch.setenv("FFTUP_LIBRARY", _lib.KNOBS_LIB_PATH)
    monkeypatch.setenv("FFTUP_EXPERIMENT", text)


def test_pinned_factorizations(monkeypatch):
    """FFTUP_EXPERIMENT keys jit_row / jit_col / jit_fused pin a factorization: other valid choices give the same pixels up to
    fp32 rounding"""
    from vkresample_amd import synth
    rgb = synth.frame(9, 640, 480, "N")

    def run():
        with _up(640, 480, 2.0, 0) as up:
            assert up.specialised_at_plan_time
            up.upload_rgb8(rgb)
            up.execute(1)
            return up.download_planar().astype(np.float64)
    ref = run()
    _knobs(monkeypatch, "jit_row=5,8,16;jit_col=15,4,8;jit_fused=192:8,10,16")
    got = run()
    assert np.percentile(np.abs(ref - got), 99.99) <= 1e-5 and np.abs(ref - got).max() <= 2e-4


def test_ring_batch_on_specialised_plan():
    """batched mode (three streams, ring of slots) on a specialised plan: every slot equals the single-frame result -- up to
    fp32 rounding: a plan without a ring cuts the frame into shorter strips (two per compute unit), and the first strip of a
    plane pairs the rows of its transforms differently (test_fused_output_independent_of_strip_length)"""
    from vkresample_amd import synth
    W, H = 720, 576
    frames = [synth.frame(20 + s, W, H, "N") for s in range(3)]
    single = []
    for f in frames:
        with _up(W, H, 2.0, 0) as up:
            up.upload_rgb8(f)
            up.execute(1)
            single.append(up.download_planar().copy())
    with _up(W, H, 2.0, 0, ring=3) as up:
        for s, f in enumerate(frames):
            up.upload_rgb8(f, slot=s)
        up.execute_ring(9, 0)
        for s in range(3):
            assert np.abs(up.download_planar(s).astype(np.float64) - single[s]).max() <= 5e-6


def test_plan_time_tuner(tmp_path, monkeypatch):
    """FFTUP_FLAG_TUNE_PLAN: the alternatives for the fused kernel's factorization are compiled and timed at plan creation,
    the decision lands in <cache dir>/wisdom.txt and the pixels stay within fp32 rounding of the untuned plan's."""
    from vkresample_amd import FLAG_TUNE_PLAN, synth
    monkeypatch.setenv("FFTUP_CACHE_DIR", str(tmp_path))
    rgb = synth.frame(5, 800, 600, "N")

    def run(flags):
        with _up(800, 600, 2.0, 0, 0.2, 0, flags) as up:
            assert up.specialised_at_plan_time
            up.upload_rgb8(rgb)
            up.execute(1)
            return up.download_planar().astype(np.float64)
    ref = run(0)
    assert not (tmp_path / "wisdom.txt").exists()
    tuned = run(FLAG_TUNE_PLAN)
    lines = (tmp_path / "wisdom.txt").read_text().strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("fused v1 ") and " 1600 4 f = " in lines[0], lines
    again = run(0)                       # reads the wisdom: same kernel as the tuned plan, bit for bit
    assert np.array_equal(tuned, again)
    assert np.percentile(np.abs(ref - tuned), 99.99) <= 1e-5 and np.abs(ref - tuned).max() <= 2e-4
    run(FLAG_TUNE_PLAN)                  # already known: no second measurement, no second line
    assert len((tmp_path / "wisdom.txt").read_text().strip().splitlines()) == 1


def test_plan_describe():
    with _up(1000, 1000, 2.0, 0) as up:
        assert up.description.startswith("specialised at plan time: row 10*10*10") and "fused 8*5*5*10" in up.description
    with _up(2048, 1024, 2.0, 0) as up:
        assert up.description.startswith("ahead-of-time power-of-two")
    with _up(256, 128, 1.25, 0) as up:                 # quarter-integer factors are specialised since round 5
        assert up.description.startswith("specialised at plan time: u1.25")
    with _up(250, 120, 1.2, 0) as up:                  # 6/5: ratios over 3, 5, 7 joined later in round 5 (the guard here: [59, 84), a row off)
        assert up.description.startswith("specialised at plan time: u6/5")
    with _up(250, 120, 1.8, 0) as up:                  # 9/5 = 18/10: the fused kernel's first radix would have to be 18
        assert up.description.startswith("size-generic")


@pytest.mark.parametrize("W,H,u", [
    (96, 72, float(np.nextafter(np.float32(4 / 3), np.float32(2)))),     # one float above the nearest float of 4/3: sizes 128 x 96 still exact
    (96, 72, float(np.nextafter(np.float32(4 / 3), np.float32(1)))),     # one below: 127 x 95 -- odd, not a configuration
    (128, 64, float(np.nextafter(np.float32(2), np.float32(3)))),        # just above 2
    (128, 64, float(np.nextafter(np.float32(2), np.float32(1)))),        # just below 2: 255 x 127
    (120, 100, float(np.nextafter(np.float32(1.5), np.float32(2)))),
    (250, 120, 1.2), (250, 120, float(np.nextafter(np.float32(1.2), np.float32(2)))),
    (200, 100, 1.6), (140, 70, 1.4), (168, 84, float(np.float32(7 / 6))), (224, 112, float(np.float32(15 / 14)))])
def test_float_factors_at_the_edges(W, H, u):
    """The factor is a float and the reference multiplies, truncates and divides in float (VR:1417, 1494-1495): a factor one ulp off a
    ratio may give the same sizes, sizes one pixel short, or a guard a row off.  Whatever the plan decides -- specialised, size-generic,
    or no configuration at all -- the result agrees with the oracle, which repeats that arithmetic."""
    import vkresample_amd as v
    from vkresample_amd import synth
    if O.check(W, H, u, 0) != 0:
        with pytest.raises(v.FftupError):
            v.Upscaler(W, H, u, 0, 0.2, 0)
        return
    rgb = synth.frame(31, W, H, "N")
    for flags in (0, v.FLAG_GENERIC_KERNELS):
        with v.Upscaler(W, H, u, 0, 0.2, 0, flags) as up:
            up.upload_rgb8(rgb)
            up.execute(1)
            pre, out = up.download_presharpen().astype(np.float64), up.download_planar().astype(np.float64)
        opre, oout, _ = O.upscale_rgb8(rgb, u, 0, 0.2)
        assert pre.shape == opre.shape
        assert np.abs(pre - opre).max() * u * u <= 1e-5 and np.abs(out - oout).max() <= 5e-4
