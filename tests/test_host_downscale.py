"""CPU: FFTUP_FLAG_DOWNSCALE is declared in the header and the binding, and plan validation of downscale plans happens before any
device access -- every case below returns the same code with or without a GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_in_header_and_binding():
    import vkresample_amd as v
    from vkresample_amd import _lib
    src = open(os.path.join(ROOT, "include", "fftup.h")).read()
    assert re.search(r"\bFFTUP_FLAG_DOWNSCALE\s*=\s*512u", src)
    assert _lib.FLAG_DOWNSCALE == 512 and v.FLAG_DOWNSCALE == 512


@pytest.mark.parametrize("W,H,u,flags", [(4096, 2048, 0.5, 0), (1920, 1080, 2 / 3, 0), (2048, 1024, 0.125, 0),
                                         (1000, 800, 0.8, 0), (640, 480, 0.75, 256), (7680, 4320, 0.5, 0)])
def test_valid_plan_passes_validation(W, H, u, flags):
    import vkresample_amd as v
    for precision in (0, 2):
        try:
            with v.Upscaler(W, H, u, precision, 0.2, 0, flags | v.FLAG_DOWNSCALE) as up:
                assert (up.out_width, up.out_height) == (int(u * W + 1e-3), int(u * H + 1e-3))
        except v.FftupError as e:
            assert e.code == 4 and v.device_count() == 0, str(e)           # FFTUP_E_NO_DEVICE: validation passed


@pytest.mark.parametrize("kwargs,code", [
    (dict(width=64, height=64, upscale=1.0), 1),            # the factor must lie in [1/8, 1)
    (dict(width=64, height=64, upscale=2.0), 1),
    (dict(width=64, height=64, upscale=0.1), 1),
    (dict(width=64, height=64, upscale=float("nan")), 1),
    (dict(width=66, height=64, upscale=0.5), 1),            # uW = 33: odd
    (dict(width=2, height=64, upscale=0.5), 1),             # uW = 1
    (dict(width=4, height=64, upscale=0.25), 1),            # uW = 1
    (dict(width=8, height=8, upscale=0.125), 1),            # uW = uH = 1
    (dict(width=1408, height=64, upscale=0.5), 2),          # uW = 704 = 2^6 * 11: not smooth
    (dict(width=64, height=88, upscale=0.5), 2),            # uH = 44 = 4 * 11
    (dict(width=64, height=64, upscale=0.5, precision=1), 3),
    (dict(width=8400, height=64, upscale=0.5), 2),          # W > 8192
    (dict(width=8400, height=64, upscale=0.5, flags=256), 2),
])
def test_invalid_plans_fail_before_device_access(kwargs, code):
    import vkresample_amd as v
    kwargs = dict(kwargs)
    kwargs["flags"] = kwargs.get("flags", 0) | v.FLAG_DOWNSCALE
    with pytest.raises(v.FftupError) as e:
        v.Upscaler(**kwargs)
    assert e.value.code == code, kwargs


def test_factor_below_one_without_the_flag_is_still_invalid():
    import vkresample_amd as v
    for flags in (0, v.FLAG_DCT, v.FLAG_GENERIC_KERNELS):
        with pytest.raises(v.FftupError) as e:
            v.Upscaler(64, 64, 0.5, 0, 0.2, 0, flags)
        assert e.value.code == 1
