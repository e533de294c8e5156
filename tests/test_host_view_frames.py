"""CPU: fftup_execute_device_views / fftup_download_view_tables are declared in the header, exported and bound; views_between; and
the fp64 phase arithmetic the device builds a frame's chirp tables with (csrc/view_phase.hpp, run by k_view_tables) agrees with the
long double host tables of csrc/view_tables.hpp / mirror_tables.hpp to one fp32 rounding step -- compiled for the host, no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vkresample_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "view_frames", "view_phase_driver.cpp")

# (N, M, origin, span, mirror): the GPU tests' axes, the workload's sizes, the longest convolution (L = 8192), origins of 1e9
# pixels at the closed bounds of the step (1/64 and 8), and large phases at a step that is no machine number (s q / n up to 1e8)
CASES = [(48, 40, 10.3, 17.9, 0), (45, 64, -3.25, 61.5, 0), (50, 32, 5.5, 77.7, 0), (46, 70, 0.4, 23.0, 1),
         (1920, 1920, 480.0, 960.0, 0), (1920, 3840, -0.25, 1920.0, 1), (4096, 4096, 0.5, 4096.0, 0), (64, 64, 1e9, 1.0, 0),
         (48, 48, -1e9, 384.0, 0), (1366, 1920, -0.144, 1366.0, 1), (6, 8186, 0.37, 65000.3, 0)]


def test_symbols_in_header_library_and_binding():
    import vkresample_amd as v
    from vkresample_amd import _lib
    src = open(os.path.join(ROOT, "include", "fftup.h")).read()
    assert re.search(r"FFTUP_API int fftup_execute_device_views\(fftup_plan\* plan, const fftup_device_image\* in, const fftup_device_image\* out,"
                     r"\s*const fftup_view\* views, uint32_t n_frames, void\* stream\);", src)
    assert re.search(r"FFTUP_API int fftup_download_view_tables\(fftup_plan\* plan, uint32_t lane, uint32_t axis, float\* pre, float\* post, "
                     r"float\* bhat, int32_t\* kmax\);", src)
    assert "fftup_execute_device_views" in _lib.EXPORTS and "fftup_download_view_tables" in _lib.EXPORTS
    lib = _lib.load()
    assert len(lib.fftup_execute_device_views.argtypes) == 6 and len(lib.fftup_download_view_tables.argtypes) == 7
    # callers detect the calls by the symbol: the ABI and the version string are the ones before they existed
    assert re.search(r"\bFFTUP_ABI_VERSION\s*=\s*2\b", src) and lib.fftup_version().decode() == "fftup 0.7.0 (gfx950, ABI 2)"
    assert callable(v.Upscaler.execute_device_views) and callable(v.Upscaler.download_view_tables) and callable(v.views_between)


def test_null_arguments_are_refused():
    from vkresample_amd import _lib
    lib = _lib.load()
    assert lib.fftup_execute_device_views(None, None, None, None, 1, None) == 1 and b"null" in lib.fftup_last_error()
    assert lib.fftup_download_view_tables(None, 0, 0, None, None, None, None) == 1 and b"null" in lib.fftup_last_error()


def test_length_mismatch_is_refused_before_the_library():
    """(an Upscaler without a plan or a library handle: anything but the ValueError would be an AttributeError)"""
    import vkresample_amd as v
    up = object.__new__(v.Upscaler)
    im = v.DeviceImage(0, v.FMT_RGB8, 0)
    view = ((0.0, 0.0), (8.0, 8.0))
    for ins, outs, views in (([im, im], [im, im], [view]), ([im], [im, im], [view, view]), ([im, im], [im], [view, view]), (im, im, [])):
        with pytest.raises(ValueError):
            v.Upscaler.execute_device_views(up, ins, outs, views)


def test_views_between():
    import vkresample_amd as v
    v0, v1 = ((10.3, 7.75), (17.9, 12.2)), ((3.0, 4.0), (8.0, 6.0))
    for n in (2, 3, 4, 7):
        got = v.views_between(v0, v1, n)
        assert len(got) == n and got[0] == v0 and got[-1] == v1                     # the ends, exactly
        for k, (o, s) in enumerate(got):
            t = k / (n - 1)
            for a in (0, 1):
                assert abs(o[a] - (v0[0][a] + t * (v1[0][a] - v0[0][a]))) <= 1e-14       # linear
                assert abs(s[a] / v0[1][a] - (v1[1][a] / v0[1][a]) ** t) <= 1e-14        # geometric
    assert v.views_between(v0, v1, 1) == [v0]
    mid = v.views_between(((0, 0), (100, 100)), ((10, 20), (400, 25)), 3)[1]
    assert mid == ((5.0, 10.0), (200.0, 50.0))


@pytest.fixture(scope="module")
def phase_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("view_frames") / "view_phase_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, DRIVER, "-o", exe])
    return exe


def _run(exe, case):
    N, M, origin, span, mirror = case
    out = subprocess.run([exe, str(N), str(M), repr(origin), repr(span), str(mirror)], capture_output=True, text=True, check=True).stdout.split("\n")
    kmax, L = (int(t) for t in out[0].split())
    rows = {t[0]: [float(x) for x in t[1:]] for t in (line.split() for line in out[1:] if line)}
    return kmax, L, rows


@pytest.mark.parametrize("case", CASES, ids=["%dto%d_o%g_s%g_m%d" % c for c in CASES])
def test_fp64_phases_against_the_long_double_tables(phase_driver, case):
    """per table the largest |difference| to make_axis / make_mirror_axis over max |table|: at most 2^-23, one fp32 rounding step --
    both sides round the same real number once, so they differ where it lies within their own error of a rounding boundary.
    (Plain fp64 s q / n loses eight digits at these phases; the compensated form keeps the difference to single flips.)"""
    kmax, L, rows = _run(phase_driver, case)
    assert set(rows) == {"pre", "post", "bhat"}
    for name, (diff, top, rel) in rows.items():
        print("MEASURED view_phase %s %s: max|diff| %.3g  max|table| %.3g  quotient %.3g (of 2^-23: %.3g)" % (case, name, diff, top, rel, rel * 2.0 ** 23))
        assert top > 0 and rel <= 2.0 ** -23, (case, name, diff, top)


def test_fp64_phases_under_the_sanitizers(tmp_path):
    """the same driver as a stand-alone program with AddressSanitizer and UBSan, on a periodic and a mirror axis"""
    exe = str(tmp_path / "view_phase_driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, DRIVER, "-o", exe])
    for case in (CASES[1], CASES[3]):
        N, M, origin, span, mirror = case
        r = subprocess.run([exe, str(N), str(M), repr(origin), repr(span), str(mirror)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
