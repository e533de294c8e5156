"""CPU: fftup_execute_device_views_shifted and fftup_shift_path are declared in the header, exported and bound; the rules of
fftup_shift_path that need no device; and the arithmetic of the path kernel (csrc/shift_path.hpp, run by k_shift_path) as a
stand-alone program under AddressSanitizer and UBSan, held to tests/path_oracle.py on the grid the GPU test runs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import path_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vkresample_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "path", "shift_path_driver.cpp")


def test_symbols_in_header_library_and_binding():
    import vkresample_amd as v
    from vkresample_amd import _lib
    src = open(os.path.join(ROOT, "include", "fftup.h")).read()
    assert re.search(r"FFTUP_API int fftup_execute_device_views_shifted\(fftup_plan\* plan, const fftup_device_image\* in, const fftup_device_image\* out,"
                     r"\s*const fftup_view\* views, const fftup_shift\* shifts_device,\s*uint32_t n_frames, void\* stream\);", src)
    assert re.search(r"FFTUP_API int fftup_shift_path\(const fftup_path_config\* cfg, const fftup_shift\* in_device, fftup_shift\* out_device,"
                     r"\s*uint32_t n_frames, void\* stream[^)]*\);", src)
    assert re.search(r"enum \{ FFTUP_PATH_ABSOLUTE = 0, FFTUP_PATH_CONSECUTIVE = 1, FFTUP_PATH_MAX_FRAMES = 4096 \};", src)
    assert re.search(r"typedef struct fftup_path_config \{ uint32_t mode; float sigma; float min_peak; \} fftup_path_config;", src)
    assert "fftup_execute_device_views_shifted" in _lib.EXPORTS and "fftup_shift_path" in _lib.EXPORTS
    lib = _lib.load()
    assert len(lib.fftup_execute_device_views_shifted.argtypes) == 7 and len(lib.fftup_shift_path.argtypes) == 5
    # callers detect the calls by the symbol: the ABI and the version string are the ones before they existed
    assert re.search(r"\bFFTUP_ABI_VERSION\s*=\s*2\b", src) and lib.fftup_version().decode() == "fftup 0.7.0 (gfx950, ABI 2)"
    assert callable(v.Upscaler.execute_device_views_shifted) and callable(v.shift_path) and callable(v.stabilised_views)
    assert (v.PATH_ABSOLUTE, v.PATH_CONSECUTIVE, v.PATH_MAX_FRAMES) == (0, 1, 4096) == (PO.ABSOLUTE, PO.CONSECUTIVE, PO.MAX_FRAMES)


def test_header_compiles_as_c_and_cxx_and_the_mirror_has_the_compilers_size(tmp_path):
    from vkresample_amd import _lib
    body = ('#include <stddef.h>\n#include <stdio.h>\n#include "fftup.h"\n'
            'int main(void){ fftup_path_config c = {FFTUP_PATH_CONSECUTIVE, 1.5f, 0.0f}; (void)c;\n'
            '  printf("%d %d %d %d\\n", (int)sizeof(fftup_path_config), (int)offsetof(fftup_path_config, sigma), (int)offsetof(fftup_path_config, min_peak), (int)FFTUP_PATH_MAX_FRAMES);\n'
            '  return FFTUP_PATH_ABSOLUTE + FFTUP_OK; }\n')
    for comp, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        f, exe = tmp_path / ("t." + ext), tmp_path / ("t_" + ext)
        f.write_text(body)
        subprocess.check_call([comp, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe)])
        got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
        assert got == [C.sizeof(_lib.PathConfig), _lib.PathConfig.sigma.offset, _lib.PathConfig.min_peak.offset, 4096] == [12, 4, 8, 4096]


def test_length_mismatch_is_refused_before_the_library():
    import vkresample_amd as v
    up = object.__new__(v.Upscaler)
    im = v.DeviceImage(0, v.FMT_RGB8, 0)
    view = ((0.0, 0.0), (8.0, 8.0))
    for ins, outs, views in (([im, im], [im, im], [view]), ([im], [im, im], [view, view]), (im, im, [])):
        with pytest.raises(ValueError):
            v.Upscaler.execute_device_views_shifted(up, ins, outs, views, 16)


def test_rules_that_need_no_device():
    """the rules on the numbers are checked ahead of any device access: every one returns code 1 and names itself"""
    import vkresample_amd as v
    from vkresample_amd import _lib
    lib = _lib.load()
    assert lib.fftup_execute_device_views_shifted(None, None, None, None, None, 1, None) == 1 and b"null" in lib.fftup_last_error()
    for n in (0, 4097):
        with pytest.raises(v.FftupError) as e:
            v.shift_path(16, 16, n)
        assert e.value.code == 1 and ("n_frames must be > 0" if n == 0 else "above FFTUP_PATH_MAX_FRAMES") in str(e.value)
    inf, nan = float("inf"), float("nan")
    for kw, text in ((dict(mode=2), "mode must be"), (dict(sigma=-0.5), "sigma must be"), (dict(sigma=nan), "sigma must be"), (dict(sigma=inf), "sigma must be"),
                     (dict(sigma=256.5), "sigma must be"), (dict(min_peak=nan), "min_peak must be"), (dict(min_peak=-inf), "min_peak must be")):
        with pytest.raises(v.FftupError) as e:
            v.shift_path(16, 16, 8, **kw)
        assert e.value.code == 1 and text in str(e.value), str(e.value)
    for a, b, text in ((None, 16, "in_device is null"), (16, None, "out_device is null")):
        with pytest.raises(v.FftupError) as e:
            v.shift_path(a, b, 8)
        assert e.value.code == 1 and text in str(e.value)
    cfg = _lib.PathConfig(0, 0.0, 0.0)
    assert lib.fftup_shift_path(None, 16, 16, 8, None) == 1 and b"cfg is null" in lib.fftup_last_error()
    assert lib.fftup_shift_path(C.byref(cfg), 18, 16, 8, None) == 1 and b"in_device is not a multiple of 4 bytes" in lib.fftup_last_error()


# ---------------------------------------------------------------- csrc/shift_path.hpp as a stand-alone program, sanitized
@pytest.fixture(scope="module")
def path_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("path") / "shift_path_driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, DRIVER, "-o", exe])
    return exe


def _drive(exe, shifts, mode, sigma, min_peak):
    text = "%d %.9g %.9g %d\n" % (mode, np.float32(sigma), np.float32(min_peak), len(shifts))
    text += "\n".join(" ".join("%x" % w for w in row) for row in np.ascontiguousarray(shifts, np.float32).view(np.uint32)) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = np.array([[float(x) for x in line.split()] for line in r.stdout.splitlines()])
    assert got.shape == (len(shifts), 6)
    return got[:, 0:2], got[:, 2:4], got[:, 4:6]


@pytest.mark.parametrize("mode", PO.MODES, ids=["absolute", "consecutive"])
def test_shift_path_hpp_against_the_oracle(path_driver, mode):
    """the grid of the GPU test, both min_peak: out within one fp32 rounding step of the oracle, 2^-23 max(|oracle|, 1); p and s
    within 1e-9.  (The driver scans in blocks of four as the kernel does, the oracle serially.)"""
    worst = [0.0, 0.0, 0.0]
    for (n, sigma) in PO.GRID:
        for min_peak in PO.MIN_PEAKS:
            sh, (p, s, out) = PO.grid_case(n, sigma, mode, min_peak)
            gp, gs, gout = _drive(path_driver, sh, mode, sigma, min_peak)
            worst = [max(worst[0], np.abs(gp - p).max()), max(worst[1], np.abs(gs - s).max()), max(worst[2], (np.abs(gout - out) / PO.out_bar(out)).max())]
            assert np.abs(gp - p).max() <= PO.P_S_BAR and np.abs(gs - s).max() <= PO.P_S_BAR, (n, sigma, min_peak)
            assert (np.abs(gout - out) <= PO.out_bar(out)).all(), (n, sigma, min_peak)
            assert np.array_equal(gout, gout.astype(np.float32).astype(np.float64))
    print("MEASURED shift_path.hpp mode %d: max |p - oracle| %.3g, |s - oracle| %.3g, |out - oracle| / bar %.3g" % (mode, *worst))
