"""CPU: FFTUP_FLAG_ODD_SIZE is declared in the header and the binding, and plan validation of odd-size plans is arithmetic on the
sizes that happens before any device access -- every case below returns the same code with or without a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (W, H, u, extra flags, (uW, uH)): at least one of W, H, uW, uH odd; every length 2,3,5,7-smooth
VALID = [(45, 21, 2.0, "", (90, 42)), (63, 35, 3.0, "", (189, 105)), (50, 30, 1.5, "", (75, 45)), (45, 32, 2.0, "", (90, 64)),
         (75, 45, 1.4, "", (105, 63)), (1215, 675, 2.0, "", (2430, 1350)), (2187, 15, 1.0, "", (2187, 15)),
         (125, 75, 0.6, "down", (75, 45))]
# ... and with a prime factor above 7 somewhere: FLAG_ANY_SIZE as well (4095 = 9 * 5 * 7 * 13: L = 8192)
VALID_ANY = [(62, 38, 1.5, "any", (93, 57)), (1365, 767, 2.0, "any", (2730, 1534)), (4095, 63, 1.0, "any", (4095, 63)),
             (2730, 1534, 0.5, "any down", (1365, 767))]


def _flags(v, extra):
    return (v.FLAG_DOWNSCALE if "down" in extra else 0) | (v.FLAG_ANY_SIZE if "any" in extra else 0)


def test_flag_value_in_header_and_binding():
    import vkresample_amd as v
    from vkresample_amd import _lib
    src = open(os.path.join(ROOT, "include", "fftup.h")).read()
    assert re.search(r"\bFFTUP_FLAG_ODD_SIZE\s*=\s*2048u", src)
    assert _lib.FLAG_ODD_SIZE == 2048 and v.FLAG_ODD_SIZE == 2048
    assert re.search(r"\bFFTUP_ABI_VERSION\s*=\s*2\b", src) and _lib.load().fftup_version().decode() == "fftup 0.7.0 (gfx950, ABI 2)"


@pytest.mark.parametrize("W,H,u,extra,out", VALID + VALID_ANY)
def test_odd_plan_passes_validation_with_the_flag(W, H, u, extra, out):
    import vkresample_amd as v
    assert out == (int(np.float32(u) * np.float32(W)), int(np.float32(u) * np.float32(H)))
    assert (W | H | out[0] | out[1]) & 1
    for precision in (0, 2):
        try:
            with v.Upscaler(W, H, u, precision, 0.2, 0, _flags(v, extra) | v.FLAG_ODD_SIZE) as up:
                assert (up.out_width, up.out_height) == out
        except v.FftupError as e:
            assert e.code == 4 and v.device_count() == 0, str(e)           # FFTUP_E_NO_DEVICE: validation passed


@pytest.mark.parametrize("W,H,u,extra,out", VALID + VALID_ANY)
def test_the_same_sizes_without_the_flag_are_invalid(W, H, u, extra, out):
    """... FLAG_ANY_SIZE alone included (62x38 -u 1.5: tests/test_host_anysize.py pins it too)"""
    import vkresample_amd as v
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(W, H, u, 0, 0.2, 0, _flags(v, extra))
    assert e.value.code == 1
    assert "must be even" in str(e.value)


@pytest.mark.parametrize("kwargs,code", [
    (dict(width=62, height=38, upscale=1.5), 2),                  # 93 = 3 * 31, 57 = 3 * 19: FLAG_ANY_SIZE is missing
    (dict(width=4097, height=63, upscale=1.0, flags=1024), 2),    # 4097 = 17 * 241, beyond 4096
    (dict(width=45, height=21, upscale=2.0, precision=1), 3),
    (dict(width=45, height=21, upscale=2.0, flags=256), 2),       # FLAG_DCT: not covered
])
def test_invalid_plans_fail_before_device_access(kwargs, code):
    import vkresample_amd as v
    kwargs = dict(kwargs)
    kwargs["flags"] = kwargs.get("flags", 0) | v.FLAG_ODD_SIZE
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(**kwargs)
    assert e.value.code == code, kwargs


def test_the_flag_is_a_no_op_on_an_even_plan():
    """2048x1024 -u 2 and neighbours: the flag does not bring the odd plans' bounds (8192x4096: non-R2C rows, long columns)"""
    import vkresample_amd as v
    for (W, H, u, flags) in [(2048, 1024, 2.0, 0), (8192, 4096, 2.0, 0), (4096, 2048, 0.5, v.FLAG_DOWNSCALE), (1366, 768, 2.0, v.FLAG_ANY_SIZE)]:
        try:
            with v.Upscaler(W, H, u, 0, 0.2, 0, flags | v.FLAG_ODD_SIZE) as up:
                assert up.out_width == int(u * W)
        except v.FftupError as e:
            assert e.code == 4 and v.device_count() == 0, str(e)
    # ... nor does it turn an unsupported even size into a supported one
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(1366, 768, 2.0, 0, 0.2, 0, v.FLAG_ODD_SIZE)
    assert e.value.code == 2


def test_jit_check_keeps_refusing_odd_sizes():
    import ctypes
    from vkresample_amd import _lib
    desc = ctypes.create_string_buffer(256)
    assert _lib.load().fftup_jit_check(1215, 675, 2.0, 0, b"", desc, 256) == 2
