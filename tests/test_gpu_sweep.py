"""GPU: seeded sweeps over sizes / upscale factors / precisions / flags (every 2,3,5,7-smooth size the reference's
scheduler accepts, vkFFT.h:4719-4726), each case against the oracle: small sizes with all factors (mostly the size-generic
kernels), and larger sizes with integer and half-integer factors (kernels specialised at plan time, csrc/jit.hpp: every case picks its own
factorizations, so this is what exercises the chooser and the N-stage engines over radix combinations nobody listed)."""
import numpy as np
import pytest

import oraclelib as O
from paritylib import smooth, within_one_half_ulp

pytestmark = pytest.mark.gpu

SMOOTH = sorted({2 ** a * 3 ** b * 5 ** c * 7 ** d for a in range(1, 10) for b in range(4) for c in range(3) for d in range(3)
                 if 4 <= 2 ** a * 3 ** b * 5 ** c * 7 ** d <= 640})


def _cases():
    import os
    rng = np.random.default_rng(int(os.environ.get("FFTUP_SWEEP_SEED", "20260930")))
    out = []
    while len(out) < int(os.environ.get("FFTUP_SWEEP_N", "144" if os.environ.get("FFTUP_BIG_TESTS", "0") != "0" else "28")):      # (a one-off 1500-case run is logged in profiles/)
        W, H = int(rng.choice(SMOOTH)), int(rng.choice(SMOOTH))
        u = float(rng.choice([1.0, 1.25, 1.5, 2.0, 2.0, 2.0, 2.5, 3.0, 4.0]))
        uW, uH = int(np.float32(u) * np.float32(W)), int(np.float32(u) * np.float32(H))
        if uW % 2 or uH % 2 or not smooth(uW) or not smooth(uH) or uW * uH > 1 << 20 or uW > 4096:
            continue
        p = int(rng.choice([0, 0, 1, 2]))
        flags = int(rng.choice([0, 2])) if p != 1 else 0
        out.append((W, H, u, p, flags, float(rng.choice([0.2, 0.2, 0.05, 0.0])), len(out)))
    return out


SMOOTH_BIG = sorted({2 ** a * 3 ** b * 5 ** c * 7 ** d for a in range(1, 12) for b in range(5) for c in range(4) for d in range(3)
                     if 64 <= 2 ** a * 3 ** b * 5 ** c * 7 ** d <= 2048})


def _cases_specialised():
    import os
    rng = np.random.default_rng(int(os.environ.get("FFTUP_SWEEP_SEED", "20260930")) + 1)
    out = []
    while len(out) < int(os.environ.get("FFTUP_SWEEP_JIT_N", "32" if os.environ.get("FFTUP_BIG_TESTS", "0") != "0" else "6")):  # (a one-off 400-case run is logged in profiles/)
        W, H = int(rng.choice(SMOOTH_BIG)), int(rng.choice(SMOOTH_BIG))
        u = float(rng.choice([2.0, 2.0, 2.0, 3.0, 4.0, 5.0, 1.5, 1.5, 2.5, 1.25, 1.75, 2.25]))
        if os.environ.get("FFTUP_SWEEP_RATIOS", "0") != "0":                    # (one-off runs: eighths and ratios over 3, 5, 7 as well)
            u = float(np.float32(rng.choice([1.125, 1.875, 4 / 3, 5 / 3, 8 / 3, 1.2, 1.4, 1.6, 8 / 7, 2.0, 1.5])))
            uW, uH = int(np.float32(u) * np.float32(W)), int(np.float32(u) * np.float32(H))
            num, den = next((round(2 * dd * u), 2 * dd) for dd in (1, 2, 4, 3, 5, 7) if abs(2 * dd * u - round(2 * dd * u)) < 1e-5 * 2 * dd * u)
            # (exact sizes, even, smooth, whole quads; the guard's float arithmetic may still say no: then the case checks the fallback's parity)
            if uW * den != num * W or uH * den != num * H or uW % 4 or uH % 2 or uW > 8192 or uW * uH > 3 << 20 or not smooth(uW) or not smooth(uH):
                continue
            p = int(rng.choice([0, 0, 2]))
            out.append((W, H, u, p, int(rng.choice([0, 2])), float(rng.choice([0.2, 0.2, 0.05])), len(out)))
            continue
        if u * W > 8192 or u * u * W * H > 3 << 20 or (2 * u * W) % 4 or (2 * u * H) % 4 or not smooth(int(u * W)) or not smooth(int(u * H)):
            continue
        if (4 * u) % 2 and ((u * W) % 4 or (u * H) % 2):                       # quarter-integer factors: whole, even output sizes
            continue
        p = int(rng.choice([0, 0, 2]))
        out.append((W, H, u, p, int(rng.choice([0, 2])), float(rng.choice([0.2, 0.2, 0.05])), len(out)))
    return out


@pytest.mark.parametrize("W,H,u,p,flags,sharpen,seed", _cases_specialised())
def test_sweep_specialised_against_oracle(W, H, u, p, flags, sharpen, seed):
    _sweep_case(W, H, u, p, flags, sharpen, seed, expect_specialised=True)


@pytest.mark.parametrize("W,H,u,p,flags,sharpen,seed", _cases())
def test_sweep_against_oracle(W, H, u, p, flags, sharpen, seed):
    _sweep_case(W, H, u, p, flags, sharpen, seed)


def _sweep_case(W, H, u, p, flags, sharpen, seed, expect_specialised=False):
    import vkresample_amd as v
    from vkresample_amd import synth
    rgb = synth.frame(1000 + seed, W, H, "N" if seed % 3 else "U")
    if O.check(W, H, u, p) != 0:
        pytest.skip("not a configuration of the reference")
    with v.Upscaler(W, H, u, p, sharpen, 0, flags) as up:
        if expect_specialised and not up.tuned:
            import ctypes as C
            from vkresample_amd import _lib
            buf = C.create_string_buffer(256)
            # the size-generic kernels are a legitimate answer only where no factorization exists
            assert _lib.load().fftup_jit_check(W, H, float(u), p, None, buf, 256) == 2, "plan fell back although a specialised plan exists"
        up.upload_rgb8(rgb)
        up.execute(1 + seed % 3)                        # one, two or three iterations (in order, one stream)
        pre = up.download_presharpen().astype(np.float64)
        out = up.download_planar().astype(np.float64)
        u8_planes = up.download_rgb8()                  # (k_pack_u8: four pixels per thread, scalar tail where 4 does not divide uW)
    if expect_specialised:
        # the fused 8-bit store of the same plan (strips per plane, the three planes' strips of the same rows 8 workgroups apart:
        # every size draws its own strip length, ragged last strips, row lengths that are no multiple of 256): the bytes of
        # planes + conversion launch, up to the few values a differently cut strip rounds to the other side of k/255
        with v.Upscaler(W, H, u, p, sharpen, 0, flags | v.FLAG_FUSE_U8_STORE) as up8:
            if up8.u8_store:
                up8.upload_rgb8(rgb)
                up8.execute(1)
                d8 = np.abs(up8.download_rgb8().astype(int) - u8_planes.astype(int))
                assert d8.max() <= 1 and (d8 != 0).sum() <= max(3, (1e-5 if p == 0 else 1e-4) * d8.size), (int(d8.max()), int((d8 != 0).sum()), d8.size)
    opre, oout, ou8 = O.upscale_rgb8(rgb, u, p, sharpen)
    # the 8-bit image: trunc(255 x) can flip by one code on a float error (for u = 1 every exact value sits ON a code boundary);
    # -p 2: one binary16 ulp near 1.0 is a quarter of a code
    d8o = np.abs(u8_planes.astype(int) - ou8.astype(int))
    assert d8o.max() <= (1 if p != 2 else 2), int(d8o.max())
    scale = 1.0 / (np.float32(u) * np.float32(u))                      # the pre-sharpen image is g / u^2
    if p == 1:
        assert np.abs(pre - opre).max() <= 1e-12
        assert np.abs(out - oout).max() <= 1e-7      # sqrt(min) has unbounded slope at 0 (see the fp32 test)
    elif p == 0:
        # (ten times what the full-size tests measure; uniform-noise frames and small sharpen factors: the filter's sqrt slope)
        assert np.abs(pre - opre).max() <= 1e-5 * scale * 4 and np.linalg.norm(pre - opre) <= 3e-6 * np.linalg.norm(opre)
        assert np.abs(out - oout).max() <= 5e-4
        # u = 1: the transform pair reproduces the 8-bit input, so every black pixel is EXACTLY 0 in the fp64 oracle and +-1e-7 on the
        # device -- the filter's sqrt(min / ..) turns that into ~3e-4 at every pixel with a black neighbour (max bound above still
        # holds); a 400-case run with another seed measured 2.35e-5 on four such cases (profiles/r03_z_sweep_400.txt)
        assert np.linalg.norm(out - oout) <= (5e-5 if u == 1.0 else 2e-5) * np.linalg.norm(oout)
    else:
        assert within_one_half_ulp(pre, opre).all()
        assert np.abs(out - oout).max() <= 1.6e-2 and np.linalg.norm(out - oout) <= 2e-3 * np.linalg.norm(oout)
