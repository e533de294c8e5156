"""CPU: fftup_plan_create_size is declared in the header, exported and bound, and its plan validation is arithmetic on the sizes
that happens before any device access -- every case below returns the same code with or without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (W, H, uW, uH, extra flags): the mixed case, an odd output row, rows M = N, columns M = N with odd lengths, the identity, the
# workload-sized anamorphic and one-axis ones; then lengths with a prime factor above 7
VALID = [(50, 32, 32, 50, ""), (40, 30, 25, 48, ""), (64, 48, 64, 72, ""), (45, 21, 64, 21, ""), (36, 20, 36, 20, ""),
         (720, 576, 1920, 1080, ""), (1440, 1080, 1920, 1080, ""), (3840, 1600, 1920, 1080, ""), (1215, 675, 2430, 1350, ""),
         (16, 16, 2, 128, ""), (512, 256, 1024, 512, ""), (1920, 1080, 3840, 2160, "")]
VALID_ANY = [(46, 22, 70, 30, "any"), (1366, 768, 1920, 1080, "any"), (4094, 64, 8192, 64, "any")]


def _flags(v, extra):
    return v.FLAG_ANY_SIZE if "any" in extra else 0


def test_symbol_in_header_library_and_binding():
    import vkresample_amd as v
    from vkresample_amd import _lib
    src = open(os.path.join(ROOT, "include", "fftup.h")).read()
    assert re.search(r"FFTUP_API int fftup_plan_create_size\(fftup_plan\*\* out, const fftup_config\* cfg,\s*uint32_t out_width, uint32_t out_height, uint32_t align\);", src)
    assert re.search(r"\bFFTUP_ALIGN_CORNER\s*=\s*0\b", src) and re.search(r"\bFFTUP_ALIGN_CENTRE\s*=\s*1\b", src)
    assert "fftup_plan_create_size" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.fftup_plan_create_size.argtypes is not None and len(lib.fftup_plan_create_size.argtypes) == 5
    assert (_lib.ALIGN_CORNER, _lib.ALIGN_CENTRE) == (0, 1) and (v.ALIGN_CORNER, v.ALIGN_CENTRE) == (0, 1)
    # the ABI and the version string are the ones before this call existed: callers detect it by the symbol
    assert re.search(r"\bFFTUP_ABI_VERSION\s*=\s*2\b", src) and lib.fftup_version().decode() == "fftup 0.7.0 (gfx950, ABI 2)"
    assert isinstance(v.Upscaler.__dict__["to_size"], classmethod)


@pytest.mark.parametrize("W,H,uW,uH,extra", VALID + VALID_ANY)
@pytest.mark.parametrize("align", [0, 1])
def test_valid_plans_pass_validation(W, H, uW, uH, extra, align):
    """FFTUP_E_NO_DEVICE on a box without a GPU: everything decided on the sizes has passed.  FLAG_ODD_SIZE and FLAG_DOWNSCALE are
    implied: accepted, and (sizes, names) stay what they are"""
    import vkresample_amd as v
    seen = []
    for precision in (0, 2):
        for more in (0, v.FLAG_ODD_SIZE | v.FLAG_DOWNSCALE):
            try:
                with v.Upscaler.to_size(W, H, uW, uH, precision, 0.2, 0, _flags(v, extra) | more, align=align) as up:
                    assert (up.width, up.height, up.out_width, up.out_height) == (W, H, uW, uH)
                    seen.append((up.kernel_names, up.num_kernels, up.tuned))
            except v.FftupError as e:
                assert e.code == 4 and v.device_count() == 0, str(e)
    assert all(s == (seen[0][0], 4, False) for s in seen)


INVALID = [
    # (kwargs of to_size, code, a word of fftup_last_error)
    (dict(width=1, height=32, out_width=2, out_height=32), 1, "at least 2"),
    (dict(width=50, height=1, out_width=50, out_height=2), 1, "at least 2"),
    (dict(width=8, height=32, out_width=1, out_height=32), 1, "at least 2"),
    (dict(width=50, height=8, out_width=50, out_height=1), 1, "at least 2"),
    (dict(width=50, height=32, out_width=0, out_height=0), 1, "at least 2"),
    (dict(width=50, height=32, out_width=32, out_height=50, align=2), 1, "align"),
    (dict(width=50, height=32, out_width=401, out_height=50), 1, "out_width"),      # above 8 N
    (dict(width=50, height=32, out_width=6, out_height=50), 1, "out_width"),        # below N / 8 = 6.25
    (dict(width=50, height=32, out_width=32, out_height=257), 1, "out_height"),
    (dict(width=50, height=34, out_width=32, out_height=4), 1, "out_height"),       # below 34 / 8 = 4.25
    (dict(width=50, height=32, out_width=32, out_height=50, precision=1), 3, "-p 0 and -p 2"),
    (dict(width=50, height=32, out_width=32, out_height=50, precision=3), 3, "precision"),
    (dict(width=50, height=32, out_width=32, out_height=50, flags=256), 2, "FFTUP_FLAG_DCT"),
    (dict(width=46, height=22, out_width=70, out_height=30), 2, "FFTUP_FLAG_ANY_SIZE"),            # 46 = 2 * 23 without the flag
    (dict(width=1366, height=768, out_width=1920, out_height=1080), 2, "FFTUP_FLAG_ANY_SIZE"),
    (dict(width=4098, height=64, out_width=4098, out_height=64, flags=1024), 2, "4096"),           # 4098 = 2 * 3 * 683
    (dict(width=8400, height=64, out_width=4200, out_height=64), 2, "8192"),                        # rows above 8192 points
    (dict(width=4200, height=64, out_width=8400, out_height=64), 2, "8192"),
    (dict(width=64, height=16384, out_width=64, out_height=8192), 2, "columns"),                    # one column of 16384 points does not fit
]


@pytest.mark.parametrize("kwargs,code,word", INVALID)
def test_invalid_plans_fail_before_device_access(kwargs, code, word):
    import vkresample_amd as v
    with pytest.raises(v.FftupError) as e:
        v.Upscaler.to_size(**kwargs)
    assert e.value.code == code, (kwargs, str(e.value))
    assert word in str(e.value), str(e.value)


def test_the_bounds_are_closed_intervals():
    import vkresample_amd as v
    for (W, H, uW, uH) in [(50, 32, 400, 256), (48, 32, 6, 4), (50, 40, 7, 5), (8192, 64, 8192, 64), (1024, 64, 8192, 64)]:
        try:
            with v.Upscaler.to_size(W, H, uW, uH) as up:
                assert (up.out_width, up.out_height) == (uW, uH)
        except v.FftupError as e:
            assert e.code == 4 and v.device_count() == 0, str(e)


def test_c_abi_null_pointers_and_channels():
    from vkresample_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.Config(50, 32, 3, 0.0, 0, 0.2, 0, 0, 1)                 # upscale = 0: ignored by this call
    assert lib.fftup_plan_create_size(None, C.byref(cfg), 32, 50, 0) == 1
    assert lib.fftup_plan_create_size(C.byref(h), None, 32, 50, 0) == 1
    assert b"null" in lib.fftup_last_error()
    for ch in (0, 1, 4):
        cfg.channels = ch
        assert lib.fftup_plan_create_size(C.byref(h), C.byref(cfg), 32, 50, 1) == 1 and not h.value
        assert b"channels" in lib.fftup_last_error()
    cfg.channels = 3
    rc = lib.fftup_plan_create_size(C.byref(h), C.byref(cfg), 32, 50, 1)
    assert rc in (0, 4)                                                # a NaN or zero cfg->upscale does not matter
    if rc == 0:
        lib.fftup_plan_destroy(h)
    cfg.upscale = float("nan")
    rc = lib.fftup_plan_create_size(C.byref(h), C.byref(cfg), 32, 50, 1)
    assert rc in (0, 4)
    if rc == 0:
        lib.fftup_plan_destroy(h)


def test_plan_create_keeps_its_rules():
    """the call with a factor refuses what it refused: a factor below 1 and odd sizes without their flags, mixed directions always"""
    import vkresample_amd as v
    for (W, H, u, flags, code, word) in [(64, 48, 0.5, 0, 1, "upscale"), (45, 21, 2.0, 0, 1, "must be even"), (50, 30, 1.5, 0, 1, "must be even"),
                                         (64, 48, 0.5, v.FLAG_ODD_SIZE, 1, "upscale"), (64, 48, 2.0, v.FLAG_DOWNSCALE, 1, "[0.125, 1)"),
                                         (46, 22, 2.0, 0, 2, "FFTUP_FLAG_ANY_SIZE")]:
        with pytest.raises(v.FftupError) as e:
            v.Upscaler(W, H, u, 0, 0.2, 0, flags)
        assert e.value.code == code and word in str(e.value), str(e.value)
    assert list(v.Upscaler.__init__.__code__.co_varnames[:9]) == ["self", "width", "height", "upscale", "precision", "sharpen", "device", "flags", "ring"]
    assert v.Upscaler.__init__.__defaults__ == (2.0, 0, 0.2, 0, 0, 1)
