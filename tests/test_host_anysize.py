"""CPU: FFTUP_FLAG_ANY_SIZE is declared in the header and the binding, plan validation of such plans is arithmetic on the sizes and
happens before any device access -- every case below returns the same code with or without a GPU -- and a numpy fp32 model of the
Bluestein kernel's arithmetic (csrc/kernels_bluestein.hpp) documents the accuracy to expect and why the chirp's phase is reduced
in integers."""
import os
import re

import numpy as np
import pytest

from paritylib import rel_l2, smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (W, H, u, extra flags): sizes with a prime factor above 7 somewhere among W, H, uW, uH
VALID = [(46, 22, 2.0, 0), (1366, 768, 2.0, 0), (640, 482, 2.0, 0), (1000, 800, 1.1, 0), (92, 44, 1.5, 0), (4094, 64, 1.0, 0),
         (2732, 1536, 0.5, "down")]


def _flags(v, extra):
    return v.FLAG_DOWNSCALE if extra == "down" else extra


def test_flag_value_in_header_and_binding():
    import vkresample_amd as v
    from vkresample_amd import _lib
    src = open(os.path.join(ROOT, "include", "fftup.h")).read()
    assert re.search(r"\bFFTUP_FLAG_ANY_SIZE\s*=\s*1024u", src)
    assert _lib.FLAG_ANY_SIZE == 1024 and v.FLAG_ANY_SIZE == 1024


@pytest.mark.parametrize("W,H,u,extra", VALID)
def test_non_smooth_plan_passes_validation_with_the_flag(W, H, u, extra):
    import vkresample_amd as v
    for precision in (0, 2):
        try:
            with v.Upscaler(W, H, u, precision, 0.2, 0, _flags(v, extra) | v.FLAG_ANY_SIZE) as up:
                assert (up.out_width, up.out_height) == (int(np.float32(u) * np.float32(W)), int(np.float32(u) * np.float32(H)))
        except v.FftupError as e:
            assert e.code == 4 and v.device_count() == 0, str(e)           # FFTUP_E_NO_DEVICE: validation passed


@pytest.mark.parametrize("W,H,u,extra", VALID)
def test_the_same_sizes_without_the_flag_are_unsupported(W, H, u, extra):
    import vkresample_amd as v
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(W, H, u, 0, 0.2, 0, _flags(v, extra))
    assert e.value.code == 2
    assert "unsupported size" in str(e.value) or "2,3,5,7" in str(e.value)


@pytest.mark.parametrize("kwargs,code", [
    (dict(width=62, height=38, upscale=1.5), 1),                 # 93 x 57: odd
    (dict(width=4098, height=64, upscale=1.0), 2),               # 4098 = 2 * 3 * 683, beyond 4096
    (dict(width=2054, height=64, upscale=2.0), 2),               # uW = 4108 = 4 * 13 * 79, beyond 4096
    (dict(width=46, height=22, upscale=2.0, precision=1), 3),
    (dict(width=46, height=22, upscale=2.0, flags=256), 2),      # FLAG_DCT: not covered
    (dict(width=92, height=44, upscale=0.5, flags=256 | 512), 2),  # ... with FLAG_DOWNSCALE neither
])
def test_invalid_plans_fail_before_device_access(kwargs, code):
    import vkresample_amd as v
    kwargs = dict(kwargs)
    kwargs["flags"] = kwargs.get("flags", 0) | v.FLAG_ANY_SIZE
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(**kwargs)
    assert e.value.code == code, kwargs


def test_smooth_plans_stay_valid_with_the_flag():
    """8192x4096 -u 2: every length smooth (non-R2C rows, long columns) -- the flag does not bring the Bluestein plans' bounds"""
    import vkresample_amd as v
    for (W, H, u, flags) in [(8192, 4096, 2.0, 0), (2048, 1024, 2.0, 0), (4096, 2048, 0.5, v.FLAG_DOWNSCALE)]:
        try:
            with v.Upscaler(W, H, u, 0, 0.2, 0, flags | v.FLAG_ANY_SIZE) as up:
                assert up.out_width == int(u * W)
        except v.FftupError as e:
            assert e.code == 4 and v.device_count() == 0, str(e)


# ---------------------------------------------------------------- the kernel's arithmetic in numpy
def _bluestein_length(N):
    L = 2 * N - 1
    while not smooth(L):
        L += 1
    return L


def _fft32(x, inverse=False):
    """numpy's own single-precision transform (complex64 in, complex64 out), unnormalised"""
    import numpy.fft as F
    y = F.ifft(x.astype(np.complex64), norm="forward") if inverse else F.fft(x.astype(np.complex64))
    return y.astype(np.complex64)


def _bluestein32(x, integer_phase=True):
    """fft_bluestein of kernels_bluestein.hpp: tables in double, rounded once to complex64, every product and transform in fp32;
    integer_phase=False forms the phase pi n^2 / N in fp32 instead (what a device-side sincos would do)"""
    N = x.shape[-1]
    L = _bluestein_length(N)
    n = np.arange(N, dtype=np.int64)
    if integer_phase:
        w = np.exp(-1j * np.pi * ((n * n) % (2 * N)).astype(np.float64) / N)
    else:
        ph = (np.float32(np.pi) * (n.astype(np.float32) * n.astype(np.float32))) / np.float32(N)        # fp32 throughout
        w = np.cos(ph.astype(np.float64)) - 1j * np.sin(ph.astype(np.float64))
    b = np.zeros(L, np.complex128)
    b[:N] = np.conj(w)
    b[L - N + 1:] = np.conj(w[1:][::-1])
    bhat = (np.fft.fft(b) / L).astype(np.complex64)
    w32 = w.astype(np.complex64)
    a = np.zeros(L, np.complex64)
    a[:N] = (x.astype(np.complex64) * w32).astype(np.complex64)
    A = (_fft32(a) * bhat).astype(np.complex64)
    c = _fft32(A, inverse=True)
    return (c[:N] * w32).astype(np.complex64)


@pytest.mark.parametrize("N", [46, 1366, 2732, 4094])
def test_bluestein_fp32_model_accuracy(N):
    """A Bluestein transform in fp32 with integer-reduced chirp tables is a few times a direct fp32 transform's error (measured
    with numpy's single-precision FFT: relative L2 5e-8 .. 1.5e-7 per transform, 2.6 .. 5.7 times the direct transform at the
    neighbouring smooth length, depending on numpy's version) -- four of them per pixel stay far below the project's 2e-6 bar
    (measured on the device: 2.5e-7 .. 3.6e-7, tests/test_gpu_anysize.py).  With the phase formed in fp32 the same model misses
    by orders of magnitude (1e-4 .. 3e-4 at N of a few thousand): pi n^2 / N reaches thousands of radians."""
    rng = np.random.default_rng(N)
    x = (rng.random(N) + 1j * rng.random(N)).astype(np.complex64)
    ref = np.fft.fft(x.astype(np.complex128))
    err = rel_l2(_bluestein32(x).astype(np.complex128), ref)
    M = N + 2
    while not smooth(M):
        M += 2
    xs = (rng.random(M) + 1j * rng.random(M)).astype(np.complex64)
    direct = rel_l2(_fft32(xs).astype(np.complex128), np.fft.fft(xs.astype(np.complex128)))
    bad = rel_l2(_bluestein32(x, integer_phase=False).astype(np.complex128), ref)
    print("MEASURED bluestein model N=%d L=%d: rel L2 %.3g, direct fp32 at %d: %.3g (ratio %.1f), fp32 phase: %.3g"
          % (N, _bluestein_length(N), err, M, direct, err / direct, bad))
    assert err < 5e-7                      # four transforms per pixel: < 2e-6, the fp32 parity bar of tests/test_gpu_downscale.py
    if N >= 1000:
        assert bad > 100 * err             # the reason for (n * n) % (2 N) in 64-bit integers
