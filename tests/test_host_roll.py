"""CPU: the host side of the roll estimates (fftup_roll_*, fftup_rotate_frames_angles; include/fftup.h) -- the header still compiles
as C and C++, the five symbols are exported and bound, the ctypes mirrors have the compiler's sizes and layout, the geometry rules
(csrc/plan_rules.cpp, roll_geometry) decide every request without a device: a stand-alone driver (tests/roll/roll_rules_driver.cpp,
its own main) compiled together with plan_rules.cpp under the address and undefined-behaviour sanitizers (host code only; nothing
sanitized is loaded into Python) runs them, and the library's own entry point gives the same answers before it looks for a device.
And what fftup_rotate_frames_angles refuses without looking at a device."""
import ctypes as C
import os
import re
import subprocess
import textwrap

import pytest

import roll_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_EXPORTS = ["fftup_roll_create", "fftup_roll_destroy", "fftup_roll_get_info", "fftup_roll_angles", "fftup_rotate_frames_angles"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", HIP_VISIBLE_DEVICES="")


def test_header_compiles_as_c_and_cxx_and_uses_the_new_types(tmp_path):
    body = ('#include "fftup.h"\nint main(void){ fftup_roll_config c = {0}; fftup_roll_angle a = {0.1f, 1.0f, 1.0f, 0.0f}; fftup_roll_info i; fftup_roll* r = 0;\n'
            '  (void)c; (void)a; (void)i; (void)r; return (int)sizeof(i.kernel_names) - 512 + (int)sizeof(a) - 16 + FFTUP_OK; }\n')
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
    assert re.search(r"FFTUP_API int fftup_roll_create\(fftup_roll\*\* out, const fftup_roll_config\* cfg\);", src)
    assert re.search(r"FFTUP_API void fftup_roll_destroy\(fftup_roll\* r\);", src)
    assert re.search(r"FFTUP_API int fftup_roll_get_info\(const fftup_roll\* r, fftup_roll_info\* info\);", src)
    assert re.search(r"FFTUP_API int fftup_roll_angles\(fftup_roll\* r, const fftup_device_image\* ref, const fftup_device_image\* cur,"
                     r"\s*uint32_t n_pairs, fftup_roll_angle\* angles_device, void\* stream", src)
    assert re.search(r"FFTUP_API int fftup_rotate_frames_angles\(fftup_rotate\* r, const fftup_device_image\* in, const fftup_device_image\* out,"
                     r"\s*const fftup_rotation\* rotations, const fftup_roll_angle\* angles_device, double gain,\s*uint32_t n_frames, void\* stream\);", src)
    assert re.search(r"typedef struct fftup_roll_angle \{ float angle, peak, peak_coarse, reserved; \} fftup_roll_angle;", src)
    # the sign, the modulus and the clamp are stated where a caller reads them
    assert "cur ~ fftup_rotate_frames(ref, +angle)" in src and "[-pi/2, pi/2)" in src and "clamped to [-pi/2, pi/2]" in src
    lib = _lib.load()
    want = {"fftup_roll_create": 2, "fftup_roll_destroy": 1, "fftup_roll_get_info": 2, "fftup_roll_angles": 6, "fftup_rotate_frames_angles": 8}
    assert sorted(want) == sorted(NEW_EXPORTS)
    for name, n in want.items():
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
    assert lib.fftup_roll_destroy.restype is None and lib.fftup_rotate_frames_angles.argtypes[5] is C.c_double
    # callers detect the feature by the symbols: the ABI and the version string are the ones before they existed
    assert re.search(r"\bFFTUP_ABI_VERSION\s*=\s*2\b", src) and lib.fftup_version().decode() == "fftup 0.7.0 (gfx950, ABI 2)"
    assert isinstance(v.Roller, type) and callable(v.Roller.angles) and callable(v.Roller.angles_device) and callable(v.Rotator.frames_angles)


def test_struct_sizes_and_layout_match_the_header(tmp_path):
    from vkresample_amd import _lib
    cfg_fields = [k for k, _ in _lib.RollConfig._fields_]
    info_fields = [k for k, _ in _lib.RollInfo._fields_]
    ang_fields = [k for k, _ in _lib.RollAngle._fields_]
    items = (["sizeof(fftup_roll_config)"] + ["offsetof(fftup_roll_config, %s)" % k for k in cfg_fields]
             + ["sizeof(fftup_roll_angle)"] + ["offsetof(fftup_roll_angle, %s)" % k for k in ang_fields]
             + ["sizeof(fftup_roll_info)"] + ["offsetof(fftup_roll_info, %s)" % k for k in info_fields])
    prog = tmp_path / "layout.c"
    prog.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "fftup.h"
        int main(void) {
            size_t v[] = { %s };
            for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) printf("%%zu ", v[i]);
            return 0;
        }""") % ", ".join(items))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    want = ([C.sizeof(_lib.RollConfig)] + [getattr(_lib.RollConfig, k).offset for k in cfg_fields]
            + [C.sizeof(_lib.RollAngle)] + [getattr(_lib.RollAngle, k).offset for k in ang_fields]
            + [C.sizeof(_lib.RollInfo)] + [getattr(_lib.RollInfo, k).offset for k in info_fields])
    assert got == want
    assert C.sizeof(_lib.RollAngle) == 16 and ang_fields == ["angle", "peak", "peak_coarse", "reserved"]
    assert cfg_fields == ["width", "height", "precision", "device", "window_w", "window_h", "decimate", "band", "angles", "upsample", "max_batch"]


# (name, (width, height, precision, window_w, window_h, decimate, band, angles, upsample, max_batch)) ->
# "ok d n_x n_y crop_x crop_y kappa n n_theta rho_min rho_max m_b K max_batch cx cy", or (code, a piece of the message that names the rule)
TABLE = [
    ("1080p", (1920, 1080, 0, 0, 0, 0, 0.0, 0, 0, 0), "ok 2 512 512 448 28 32 512 512 64 256 128 256 16 256 256"),
    ("2160p", (3840, 2160, 0, 0, 0, 0, 0.0, 0, 0, 0), "ok 4 512 512 896 56 32 512 512 64 256 128 256 16 256 256"),
    ("80x48", (80, 48, 0, 0, 0, 0, 0.0, 0, 0, 0), "ok 1 64 32 8 8 32 32 32 4 16 8 16 16 32 16"),
    ("160x160_auto", (160, 160, 0, 0, 0, 0, 0.0, 0, 0, 0), "ok 1 128 128 16 16 32 128 128 16 64 32 64 16 64 64"),
    ("320x192_d2", (320, 192, 0, 128, 64, 2, 0.0, 0, 0, 0), "ok 2 128 64 32 32 32 64 64 8 32 16 32 16 64 32"),
    ("explicit", (600, 300, 2, 512, 256, 1, 1.0, 1024, 8, 3), "ok 1 512 256 44 22 8 256 1024 64 256 256 512 3 512 256"),
    ("narrow_band_keeps_two_radii", (80, 48, 0, 64, 32, 1, 0.1, 0, 0, 0), "ok 1 64 32 8 8 32 32 32 2 3 8 16 16 6 3"),
    ("16k_frame_caps_the_window", (16384, 16384, 0, 0, 0, 0, 0.0, 0, 0, 0), "ok 8 512 512 6144 6144 32 512 512 64 256 128 256 16 256 256"),
    ("window_too_large", (80, 48, 0, 128, 32, 1, 0.0, 0, 0, 0), (1, "window_w * d = 128 exceeds the frame's width 80")),
    ("window_too_large_after_decimation", (160, 96, 0, 64, 64, 2, 0.0, 0, 0, 0), (1, "window_h * d = 128 exceeds the frame's height 96")),
    ("window_not_a_power_of_two", (200, 200, 0, 96, 64, 0, 0.0, 0, 0, 0), (1, "window_w 96 must be a power of two in [32, 512]")),
    ("window_16", (200, 200, 0, 64, 16, 0, 0.0, 0, 0, 0), (1, "window_h 16 must be a power of two in [32, 512]")),
    ("window_above_512", (4096, 4096, 0, 1024, 64, 0, 0.0, 0, 0, 0), (1, "window_w 1024 must be a power of two in [32, 512]")),
    ("decimate_3", (200, 200, 0, 0, 0, 3, 0.0, 0, 0, 0), (1, "decimate 3 must be 1, 2, 4 or 8")),
    ("band_1.5", (200, 200, 0, 0, 0, 0, 1.5, 0, 0, 0), (1, "band must lie in (0, 1]")),
    ("band_negative", (200, 200, 0, 0, 0, 0, -0.25, 0, 0, 0), (1, "band must lie in (0, 1]")),
    ("band_leaves_no_radius", (80, 48, 0, 64, 32, 1, 0.05, 0, 0, 0), (1, "leaves no radius")),
    ("angles_48", (200, 200, 0, 0, 0, 0, 0.0, 48, 0, 0), (1, "angles 48 must be a power of two in [32, 1024]")),
    ("angles_16", (200, 200, 0, 0, 0, 0, 0.0, 16, 0, 0), (1, "angles 16 must be a power of two in [32, 1024]")),
    ("angles_2048", (200, 200, 0, 0, 0, 0, 0.0, 2048, 0, 0), (1, "angles 2048 must be a power of two in [32, 1024]")),
    ("frame_24x24", (24, 24, 0, 0, 0, 0, 0.0, 0, 0, 0), (1, "fewer than 32 decimated pixels on an axis")),
    ("frame_too_small_after_decimation", (200, 200, 0, 0, 0, 8, 0.0, 0, 0, 0), (1, "fewer than 32 decimated pixels on an axis")),
    ("upsample_2", (200, 200, 0, 0, 0, 0, 0.0, 0, 2, 0), (1, "upsample 2 must lie in [4, 64]")),
    ("upsample_65", (200, 200, 0, 0, 0, 0, 0.0, 0, 65, 0), (1, "upsample 65 must lie in [4, 64]")),
    ("max_batch_65536", (200, 200, 0, 0, 0, 0, 0.0, 0, 0, 65536), (1, "max_batch must be <= 65535")),
    ("precision_1", (200, 200, 1, 0, 0, 0, 0.0, 0, 0, 0), (3, "precision must be 0 (float planes) or 2 (half planes)")),
    ("precision_3", (200, 200, 3, 0, 0, 0, 0.0, 0, 0, 0), (3, "precision must be 0 (float planes) or 2 (half planes)")),
    ("zero_size", (0, 200, 0, 0, 0, 0, 0.0, 0, 0, 0), (1, "width and height must be > 0")),
    ("size_above_65536", (70000, 200, 0, 0, 0, 0, 0.0, 0, 0, 0), (1, "width/height above 65536")),
]


@pytest.fixture(scope="module")
def driver_lines(tmp_path_factory):
    """the driver and plan_rules.cpp, compiled with the sanitizers for the host, the rest linked from the library's own object
    files; run once over the table"""
    d = tmp_path_factory.mktemp("roll_rules")
    exe = os.path.join(str(d), "roll_rules_driver")
    obj = os.path.join(ROOT, "build", "obj")
    objs = sorted(os.path.join(obj, f) for f in os.listdir(obj) if f.endswith(".o") and f not in ("jit_knobs.o", "plan_rules.o"))
    csrc = os.path.join(ROOT, "vkresample_amd", "csrc")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wno-option-ignored",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc,
                           "-x", "hip", os.path.join(ROOT, "tests", "roll", "roll_rules_driver.cpp"), os.path.join(csrc, "plan_rules.cpp"),
                           "-x", "none"] + objs + ["-fsanitize=address,undefined", "-o", exe])
    lines = [" ".join(str(x) if not isinstance(x, float) else float(x).hex() for x in row[1]) for row in TABLE]
    # HIP_VISIBLE_DEVICES empty: the rules must not need a device even where there is one
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=SAN_ENV)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.splitlines()
    assert len(out) == len(TABLE)
    return dict(zip([r[0] for r in TABLE], out))


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_geometry_table_without_a_device(row, driver_lines):
    name, request, want = row
    got = driver_lines[name]
    if isinstance(want, str):
        assert got == want
        v = [int(x) for x in got.split()[1:]]
        nx, ny, n, nt, rho_min, rho_max, mb, K, cx, cy = v[1], v[2], v[6], v[7], v[8], v[9], v[10], v[11], v[13], v[14]
        assert n == min(nx, ny) and mb == nt // 4 and K == 2 * mb and rho_min == max(2, rho_max // 4) and rho_min <= rho_max <= n
        assert cx == rho_max * nx // n <= nx and cy == rho_max * ny // n <= ny       # the band's columns and rows lie within the padded transform
        assert 2 * max(nx, ny, nt // 2) <= 1024                                        # the longest line of the LDS transforms
    else:
        code, piece = want
        assert got.startswith("error %d " % code) and piece in got, got


@pytest.mark.parametrize("row", [r for r in TABLE if isinstance(r[2], str)], ids=[r[0] for r in TABLE if isinstance(r[2], str)])
def test_oracle_geometry_is_the_librarys(row):
    name, rq, want = row
    g = R.geometry(rq[0], rq[1], (rq[3], rq[4]) if rq[3] else None, rq[5], rq[6], rq[7], rq[8])
    v = want.split()[1:14]
    assert [str(g[k]) for k in ("d", "nx", "ny", "crop_x", "crop_y", "kappa", "n", "angles", "rho_min", "rho_max", "mb", "K")] == v[:12]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_library_decides_the_same_before_any_device_access(row):
    """fftup_roll_create: a refused request gets its code and message with or without a device; a valid one gets as far as the
    device (FFTUP_E_NO_DEVICE where there is none)"""
    from vkresample_amd import _lib
    name, rq, want = row
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.RollConfig(rq[0], rq[1], rq[2], 0, rq[3], rq[4], rq[5], rq[6], rq[7], rq[8], rq[9])
    code = lib.fftup_roll_create(C.byref(h), C.byref(cfg))
    text = lib.fftup_last_error().decode()
    if isinstance(want, str):
        if lib.fftup_device_count() > 0:
            assert code == 0, text
            info = _lib.RollInfo()
            assert lib.fftup_roll_get_info(h, C.byref(info)) == 0
            assert "ok %d %d %d %d %d %d %d %d %d %d %d %d %d" % (info.decimate, info.window_w, info.window_h, info.crop_x, info.crop_y, info.upsample, info.n,
                                                                 info.angles, info.rho_min, info.rho_max, info.m_band, info.K, info.max_batch) == " ".join(want.split()[:14])
            names = [bytes(n).split(b"\0")[0] for n in info.kernel_names][:info.num_kernels]
            assert names == [b"roll_rows", b"roll_cols", b"roll_polar", b"roll_peak"] and info.device_bytes > 0
            lib.fftup_roll_destroy(h)
        else:
            assert code == 4, text
    else:
        assert code == want[0] and want[1] in text, (code, text)
        assert not h.value


def test_null_arguments():
    from vkresample_amd import _lib
    lib = _lib.load()
    cfg = _lib.RollConfig(80, 48, 0, 0, 0, 0, 0, 0.0, 0, 0, 0)
    h = C.c_void_p()
    assert lib.fftup_roll_create(None, C.byref(cfg)) == 1 and lib.fftup_roll_create(C.byref(h), None) == 1
    assert lib.fftup_roll_get_info(None, None) == 1
    assert lib.fftup_roll_angles(None, None, None, 1, None, None) == 1 and "null estimator" in lib.fftup_last_error().decode()
    lib.fftup_roll_destroy(None)                                     # no-op


def test_rotate_frames_angles_refusals_that_need_no_device():
    """the arguments of its own are checked first, the shared ones of fftup_rotate_frames next: none of these reaches a device"""
    from vkresample_amd import _lib
    lib = _lib.load()
    d = (_lib.DeviceImageDesc * 1)()
    rot = (_lib.Rotation * 1)(_lib.Rotation(0.0, 1.0, 1.0))
    fake = C.c_void_p(4096)                                          # never dereferenced: every call below is refused before that
    calls = [
        ((None, d, d, rot, None, -1.0, 1, None), "fftup_rotate_frames_angles: angles_device is null"),
        ((None, d, d, rot, fake, float("nan"), 1, None), "fftup_rotate_frames_angles: gain is not finite"),
        ((None, d, d, rot, fake, float("inf"), 1, None), "fftup_rotate_frames_angles: gain is not finite"),
        ((None, d, d, rot, C.c_void_p(4098), -1.0, 1, None), "fftup_rotate_frames_angles: angles_device is not a multiple of 4 bytes"),
        ((None, d, d, rot, fake, -1.0, 1, None), "fftup_rotate_frames_angles: null rotator"),
    ]
    for args, piece in calls:
        assert lib.fftup_rotate_frames_angles(*args) == 1
        assert piece in lib.fftup_last_error().decode(), (piece, lib.fftup_last_error().decode())
