"""CPU: the host side of the shift estimates (fftup_align_*, include/fftup.h) -- the header still compiles as C and C++, the four
symbols are exported and bound, the ctypes mirrors have the compiler's sizes, and the geometry rules (csrc/plan_rules.cpp,
align_geometry) decide every request without a device: a stand-alone driver (tests/align_rules_driver.cpp) linked from the library's
object files runs them, and the library's own entry point gives the same answers before it looks for a device."""
import ctypes as C
import os
import re
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_EXPORTS = ["fftup_align_create", "fftup_align_destroy", "fftup_align_get_info", "fftup_align_shifts"]


def test_header_compiles_as_c_and_cxx_and_uses_the_new_types(tmp_path):
    body = ('#include "fftup.h"\nint main(void){ fftup_align_config c = {0}; fftup_shift s = {0, 0, 0, 0}; fftup_align_info i; fftup_align* a = 0;\n'
            '  (void)c; (void)s; (void)i; (void)a; return (int)sizeof(i.kernel_names) - 512 + FFTUP_OK; }\n')
    for comp, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        f = tmp_path / ("t." + ext)
        f.write_text(body.replace("{0}", "{0}" if ext == "c" else "{}"))
        subprocess.check_call([comp, std, "-Wall", "-Werror", "-Wno-missing-braces", "-Wno-missing-field-initializers", "-I", os.path.join(ROOT, "include"),
                               str(f), "-o", str(tmp_path / ("t_" + ext))])
        assert subprocess.call([str(tmp_path / ("t_" + ext))]) == 0


def test_symbols_in_header_library_and_binding():
    import vkresample_amd as v
    from vkresample_amd import _lib
    src = open(os.path.join(ROOT, "include", "fftup.h")).read()
    assert re.search(r"FFTUP_API int fftup_align_create\(fftup_align\*\* out, const fftup_align_config\* cfg\);", src)
    assert re.search(r"FFTUP_API void fftup_align_destroy\(fftup_align\* a\);", src)
    assert re.search(r"FFTUP_API int fftup_align_get_info\(const fftup_align\* a, fftup_align_info\* info\);", src)
    assert re.search(r"FFTUP_API int fftup_align_shifts\(fftup_align\* a, const fftup_device_image\* ref, const fftup_device_image\* cur,"
                     r"\s*uint32_t n_pairs, fftup_shift\* shifts_device, void\* stream", src)
    assert "cur(x, y) ~ ref(x - dx, y - dy)" in src          # the meaning of the result, in one sentence
    lib = _lib.load()
    want = {"fftup_align_create": 2, "fftup_align_destroy": 1, "fftup_align_get_info": 2, "fftup_align_shifts": 6}
    assert sorted(want) == sorted(NEW_EXPORTS)
    for name, n in want.items():
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
    assert lib.fftup_align_destroy.restype is None
    # callers detect the feature by the symbols: the ABI and the version string are the ones before they existed
    assert re.search(r"\bFFTUP_ABI_VERSION\s*=\s*2\b", src) and lib.fftup_version().decode() == "fftup 0.7.0 (gfx950, ABI 2)"
    assert isinstance(v.Aligner, type) and callable(v.Aligner.shifts) and callable(v.Aligner.shifts_device) and callable(v.stabilised_views)
    assert v.stabilised_views(((1.0, 2.0), (40.0, 36.0)), [(0.5, -0.25, 1.0, 1.0)]) == [((1.5, 1.75), (40.0, 36.0))]


def test_struct_sizes_match_the_header(tmp_path):
    from vkresample_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "fftup.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(fftup_align_config), offsetof(fftup_align_config, band),
                   offsetof(fftup_align_config, max_batch), sizeof(fftup_shift), sizeof(fftup_align_info),
                   offsetof(fftup_align_info, num_kernels), offsetof(fftup_align_info, device_bytes), offsetof(fftup_align_info, kernel_names));
            return 0;
        }"""))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(_lib.AlignConfig), _lib.AlignConfig.band.offset, _lib.AlignConfig.max_batch.offset, C.sizeof(_lib.Shift),
                   C.sizeof(_lib.AlignInfo), _lib.AlignInfo.num_kernels.offset, _lib.AlignInfo.device_bytes.offset,
                   _lib.AlignInfo.kernel_names.offset]
    assert C.sizeof(_lib.Shift) == 16


# (name, width, height, precision, window_w, window_h, decimate, band, upsample, max_batch) -> "ok d n_x n_y crop_x crop_y kappa band_kx
# band_ky", or (code, a piece of the message that names the rule)
TABLE = [
    ("1080p", (1920, 1080, 0, 0, 0, 0, 0.0, 0, 0), "ok 1 1024 1024 448 28 32 256 256"),
    ("2160p", (3840, 2160, 0, 0, 0, 0, 0.0, 0, 0), "ok 2 1024 1024 896 56 32 256 256"),
    ("80x48", (80, 48, 0, 0, 0, 0, 0.0, 0, 0), "ok 1 64 32 8 8 32 16 8"),
    ("explicit", (600, 300, 2, 512, 256, 1, 1.0, 8, 3), "ok 1 512 256 44 22 8 256 128"),
    ("16k_frame_caps_the_window", (16384, 16384, 0, 0, 0, 0, 0.0, 0, 0), "ok 8 1024 1024 4096 4096 32 256 256"),
    ("window_too_large", (80, 48, 0, 128, 32, 1, 0.0, 0, 0), (1, "window_w * d = 128 exceeds the frame's width 80")),
    ("window_too_large_after_decimation", (160, 96, 0, 64, 64, 2, 0.0, 0, 0), (1, "window_h * d = 128 exceeds the frame's height 96")),
    ("window_not_a_power_of_two", (200, 200, 0, 96, 64, 0, 0.0, 0, 0), (1, "window_w 96 must be a power of two in [16, 1024]")),
    ("window_above_1024", (4096, 4096, 0, 2048, 64, 0, 0.0, 0, 0), (1, "window_w 2048 must be a power of two in [16, 1024]")),
    ("decimate_3", (200, 200, 0, 0, 0, 3, 0.0, 0, 0), (1, "decimate 3 must be 1, 2, 4 or 8")),
    ("band_1.5", (200, 200, 0, 0, 0, 0, 1.5, 0, 0), (1, "band must lie in (0, 1]")),
    ("band_negative", (200, 200, 0, 0, 0, 0, -0.25, 0, 0), (1, "band must lie in (0, 1]")),
    ("frame_12x12", (12, 12, 0, 0, 0, 0, 0.0, 0, 0), (1, "fewer than 16 decimated pixels on an axis")),
    ("frame_too_small_after_decimation", (100, 100, 0, 0, 0, 8, 0.0, 0, 0), (1, "fewer than 16 decimated pixels on an axis")),
    ("upsample_2", (200, 200, 0, 0, 0, 0, 0.0, 2, 0), (1, "upsample 2 must lie in [4, 64]")),
    ("precision_1", (200, 200, 1, 0, 0, 0, 0.0, 0, 0), (3, "precision must be 0 (float planes) or 2 (half planes)")),
    ("zero_size", (0, 200, 0, 0, 0, 0, 0.0, 0, 0), (1, "width and height must be > 0")),
]


@pytest.fixture(scope="module")
def driver_lines(tmp_path_factory):
    """the driver, linked from the library's own object files, run once over the table"""
    d = tmp_path_factory.mktemp("align_rules")
    exe = os.path.join(str(d), "align_rules_driver")
    obj = os.path.join(ROOT, "build", "obj")
    objs = sorted(os.path.join(obj, f) for f in os.listdir(obj) if f.endswith(".o") and f != "jit_knobs.o")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "vkresample_amd", "csrc"),
                           "-x", "hip", os.path.join(ROOT, "tests", "align_rules_driver.cpp"), "-x", "none"] + objs + ["-o", exe])
    lines = [" ".join(str(x) if not isinstance(x, float) else float(x).hex() for x in row[1]) for row in TABLE]
    # HIP_VISIBLE_DEVICES empty: the rules must not need a device even where there is one
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = p.stdout.splitlines()
    assert len(out) == len(TABLE)
    return dict(zip([r[0] for r in TABLE], out))


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_geometry_table_without_a_device(row, driver_lines):
    name, request, want = row
    got = driver_lines[name]
    if isinstance(want, str):
        assert got == want
    else:
        code, piece = want
        assert got.startswith("error %d " % code) and piece in got, got


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_library_decides_the_same_before_any_device_access(row):
    """fftup_align_create: a refused request gets its code and message with or without a device; a valid one gets as far as the
    device (FFTUP_E_NO_DEVICE where there is none)"""
    from vkresample_amd import _lib
    name, rq, want = row
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.AlignConfig(rq[0], rq[1], rq[2], 0, rq[3], rq[4], rq[5], rq[6], rq[7], rq[8])
    code = lib.fftup_align_create(C.byref(h), C.byref(cfg))
    text = lib.fftup_last_error().decode()
    if isinstance(want, str):
        if lib.fftup_device_count() > 0:
            if name == "16k_frame_caps_the_window":           # (a valid request; its frames are nothing a test needs to allocate for)
                assert code in (0, 6), text
            else:
                assert code == 0, text
            if code == 0:
                info = _lib.AlignInfo()
                assert lib.fftup_align_get_info(h, C.byref(info)) == 0
                assert "ok %d %d %d %d %d %d %d %d" % (info.decimate, info.window_w, info.window_h, info.crop_x, info.crop_y, info.upsample,
                                                      info.band_kx, info.band_ky) == want
                assert info.num_kernels == 5 and bytes(info.kernel_names[0]).split(b"\0")[0] == b"align_rows" and info.device_bytes > 0
                lib.fftup_align_destroy(h)
        else:
            assert code == 4, text
    else:
        assert code == want[0] and want[1] in text, (code, text)
        assert not h.value


def test_null_arguments():
    from vkresample_amd import _lib
    lib = _lib.load()
    cfg = _lib.AlignConfig(80, 48, 0, 0, 0, 0, 0, 0.0, 0, 0)
    h = C.c_void_p()
    assert lib.fftup_align_create(None, C.byref(cfg)) == 1 and lib.fftup_align_create(C.byref(h), None) == 1
    assert lib.fftup_align_get_info(None, None) == 1
    assert lib.fftup_align_shifts(None, None, None, 1, None, None) == 1 and "null aligner" in lib.fftup_last_error().decode()
    lib.fftup_align_destroy(None)                                    # no-op
