"""CPU: the host side of the rotation by three shears (fftup_rotate_*, include/fftup.h) -- the header still compiles as C and C++,
the four symbols are exported and bound, the ctypes mirrors have the compiler's sizes, the geometry rules (csrc/plan_rules.cpp,
rotate_geometry) decide every request without a device: a stand-alone driver (tests/rotate/rotate_rules_driver.cpp) linked from the
library's object files runs them, and the library's own entry point gives the same answers before it looks for a device.  And the
phase arithmetic the kernels run (csrc/rotate_phase.hpp), compiled for the host into a stand-alone driver
(tests/rotate/rotate_phase_driver.cpp, with the address and undefined-behaviour sanitizers, as tests/test_sanitize.py builds its
drivers), against exact rational phases evaluated in numpy's extended precision."""
import ctypes as C
import os
import re
import subprocess
import textwrap
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_EXPORTS = ["fftup_rotate_create", "fftup_rotate_destroy", "fftup_rotate_get_info", "fftup_rotate_frames"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_header_compiles_as_c_and_cxx_and_uses_the_new_types(tmp_path):
    body = ('#include "fftup.h"\nint main(void){ fftup_rotate_config c = {0}; fftup_rotation t = {0.1, 2.0, 3.0}; fftup_rotate_info i; fftup_rotate* r = 0;\n'
            '  (void)c; (void)t; (void)i; (void)r; return (int)sizeof(i.kernel_names) - 256 + FFTUP_OK; }\n')
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
    assert re.search(r"FFTUP_API int fftup_rotate_create\(fftup_rotate\*\* out, const fftup_rotate_config\* cfg\);", src)
    assert re.search(r"FFTUP_API void fftup_rotate_destroy\(fftup_rotate\* r\);", src)
    assert re.search(r"FFTUP_API int fftup_rotate_get_info\(const fftup_rotate\* r, fftup_rotate_info\* info\);", src)
    assert re.search(r"FFTUP_API int fftup_rotate_frames\(fftup_rotate\* r, const fftup_device_image\* in, const fftup_device_image\* out,"
                     r"\s*const fftup_rotation\* rotations, uint32_t n_frames, void\* stream", src)
    # the meaning of the result, the wrap-around and the 8-bit rounding are stated where a caller reads them
    assert "out(p) ~ in(c + R(-theta)(p - c))" in src and "clockwise on screen" in src
    assert "wraps around" in src and "clamp(floor(255 x + 0.5), 0, 255)" in src
    lib = _lib.load()
    want = {"fftup_rotate_create": 2, "fftup_rotate_destroy": 1, "fftup_rotate_get_info": 2, "fftup_rotate_frames": 6}
    assert sorted(want) == sorted(NEW_EXPORTS)
    for name, n in want.items():
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
    assert lib.fftup_rotate_destroy.restype is None
    # callers detect the feature by the symbols: the ABI and the version string are the ones before they existed
    assert re.search(r"\bFFTUP_ABI_VERSION\s*=\s*2\b", src) and lib.fftup_version().decode() == "fftup 0.7.0 (gfx950, ABI 2)"
    assert isinstance(v.Rotator, type) and callable(v.Rotator.rotate) and callable(v.Rotator.rotation)


def test_struct_sizes_match_the_header(tmp_path):
    from vkresample_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "fftup.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(fftup_rotate_config), offsetof(fftup_rotate_config, device),
                   offsetof(fftup_rotate_config, max_batch), sizeof(fftup_rotation), offsetof(fftup_rotation, centre_y),
                   sizeof(fftup_rotate_info), offsetof(fftup_rotate_info, max_batch), offsetof(fftup_rotate_info, device_bytes),
                   offsetof(fftup_rotate_info, kernel_names));
            return 0;
        }"""))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(_lib.RotateConfig), _lib.RotateConfig.device.offset, _lib.RotateConfig.max_batch.offset, C.sizeof(_lib.Rotation),
                   _lib.Rotation.centre_y.offset, C.sizeof(_lib.RotateInfo), _lib.RotateInfo.max_batch.offset,
                   _lib.RotateInfo.device_bytes.offset, _lib.RotateInfo.kernel_names.offset]
    assert C.sizeof(_lib.Rotation) == 24


# (name, (width, height, precision, max_batch)) -> "ok max_batch TK lds_x lds_y", or (code, pieces of the message that name the rule)
TABLE = [
    ("1080p", (1920, 1080, 0, 0), "ok 4 4 65296 73456"),
    ("45x21_odd", (45, 21, 0, 0), "ok 4 4 1536 1440"),
    ("4096x16", (4096, 16, 0, 0), "ok 4 4 139280 1104"),
    ("16x4096_half_batch_64", (16, 4096, 2, 64), "ok 64 2 560 139280"),
    ("2048_rows_keep_four_columns", (30, 2048, 0, 1), "ok 1 4 1024 139280"),
    ("4100x16_above_4096", (4100, 16, 0, 0), (2, ["width 4100 is above 4096"])),
    ("16x8192_above_4096", (16, 8192, 0, 0), (2, ["height 8192 is above 4096"])),
    ("46x22_not_smooth", (46, 22, 0, 0), (2, ["width 46 has a prime factor above 7"])),
    ("60x22_not_smooth", (60, 22, 0, 0), (2, ["height 22 has a prime factor above 7"])),
    ("1x8", (1, 8, 0, 0), (2, ["width 1 is below 2"])),
    ("8x0", (8, 0, 0, 0), (2, ["height 0 is below 2"])),
    ("precision_1", (64, 32, 1, 0), (3, ["precision must be 0 (float planes) or 2 (half planes)"])),
    ("max_batch_65", (64, 32, 0, 65), (1, ["max_batch 65 must be <= 64"])),
]


@pytest.fixture(scope="module")
def driver_lines(tmp_path_factory):
    """the driver, linked from the library's own object files, run once over the table"""
    d = tmp_path_factory.mktemp("rotate_rules")
    exe = os.path.join(str(d), "rotate_rules_driver")
    obj = os.path.join(ROOT, "build", "obj")
    objs = sorted(os.path.join(obj, f) for f in os.listdir(obj) if f.endswith(".o") and f != "jit_knobs.o")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "vkresample_amd", "csrc"),
                           "-x", "hip", os.path.join(ROOT, "tests", "rotate", "rotate_rules_driver.cpp"), "-x", "none"] + objs + ["-o", exe])
    lines = [" ".join(str(x) for x in row[1]) for row in TABLE]
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
        lds_x, lds_y = (int(x) for x in got.split()[3:])
        assert max(lds_x, lds_y) <= 160 * 1024                       # the LDS of a gfx950 compute unit
    else:
        code, pieces = want
        assert got.startswith("error %d " % code) and all(p in got for p in pieces), got


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_library_decides_the_same_before_any_device_access(row):
    """fftup_rotate_create: a refused request gets its code and message with or without a device; a valid one gets as far as the
    device (FFTUP_E_NO_DEVICE where there is none)"""
    from vkresample_amd import _lib
    name, rq, want = row
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.RotateConfig(rq[0], rq[1], rq[2], 0, rq[3])
    code = lib.fftup_rotate_create(C.byref(h), C.byref(cfg))
    text = lib.fftup_last_error().decode()
    if isinstance(want, str):
        if lib.fftup_device_count() > 0:
            assert code == 0, text
            info = _lib.RotateInfo()
            assert lib.fftup_rotate_get_info(h, C.byref(info)) == 0
            assert (info.width, info.height, info.max_batch) == (rq[0], rq[1], int(want.split()[1]))
            assert info.num_kernels == 3 and bytes(info.kernel_names[1]).split(b"\0")[0] == b"rotate_shear_y"
            assert info.device_bytes >= 2 * 12 * info.max_batch * rq[0] * rq[1]
            lib.fftup_rotate_destroy(h)
        else:
            assert code == 4, text
    else:
        assert code == want[0] and all(p in text for p in want[1]), (code, text)
        assert not h.value


def test_null_arguments():
    from vkresample_amd import _lib
    lib = _lib.load()
    cfg = _lib.RotateConfig(64, 32, 0, 0, 0)
    h = C.c_void_p()
    assert lib.fftup_rotate_create(None, C.byref(cfg)) == 1 and lib.fftup_rotate_create(C.byref(h), None) == 1
    assert lib.fftup_rotate_get_info(None, None) == 1
    assert lib.fftup_rotate_frames(None, None, None, None, 1, None) == 1 and "null rotator" in lib.fftup_last_error().decode()
    lib.fftup_rotate_destroy(None)                                   # no-op


# ---------------------------------------------------------------------------------------------------- csrc/rotate_phase.hpp
@pytest.fixture(scope="module")
def phase_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rotate_phase") / "rotate_phase_driver")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I", os.path.join(ROOT, "vkresample_amd", "csrc"),
                                                         os.path.join(ROOT, "tests", "rotate", "rotate_phase_driver.cpp"), "-o", exe])
    return exe


def _run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=SAN_ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def _exact_factor(k, n, delta):
    """bin k of a line of n points moved by `delta` (a double, taken exactly): (re, im) in extended precision and |t| in turns.
    The phase is reduced in rational arithmetic, so nothing is lost before the sine and cosine."""
    L = np.longdouble
    pi = 4 * np.arctan(L(1))
    d = Fraction(delta)

    def ld(q):                                                # a rational of magnitude <= 1 -> long double, to 2^-106
        hi = float(q)
        return L(hi) + L(float(q - Fraction(hi)))
    if 2 * k == n:
        r = d - 2 * round(d / 2)
        return np.cos(pi * ld(r)), L(0), 0.0
    f = k if 2 * k < n else k - n
    t = Fraction(f) * d / n
    r = t - round(t)
    return np.cos(2 * pi * ld(r)), -np.sin(2 * pi * ld(r)), abs(float(t))


PHASE_CASES = [
    (4096, 2047.37, [0, 1, 2047, 2048, 2049, 4095, 1000, 3333]),
    (4096, -2047.37, [0, 1, 2047, 2048, 2049, 4095, 1024, 3072]),
    (4096, 0.5, [1, 1024, 2048, 3072, 4095]),                 # quarter and half turns: exact zeros
    (1080, 311.0625, [1, 7, 539, 540, 541, 1079]),
    (45, -17.3, list(range(45))),                             # odd: no Nyquist bin
    (2, 0.25, [0, 1]),
    (64, 3.0, [0, 5, 32, 63]),                                # a whole-pixel move: the Nyquist factor is -1
]


@pytest.mark.parametrize("case", PHASE_CASES, ids=["%d_%g" % c[:2] for c in PHASE_CASES])
def test_phases_against_extended_precision(phase_driver, case):
    """every factor within ONE fp32 rounding step of the exact value (the kernels round the double pair once), plus what forming
    t = f delta / n in double may cost before the reduction: two roundings of 2^-53 relative, 2 pi |t| 2^-52 in the phase --
    1.4e-12 at the thousand turns of n = 4096, delta = 2047.37, f = 2047, where fp32 phases would be noise.  The reference's own
    sine and cosine are good to 1e-18 (a 64-bit significand, arguments up to pi): where the exact value is zero it says 2.5e-20"""
    n, delta, bins = case
    lines = _run(phase_driver, [n, float(delta).hex()] + bins)
    assert len(lines) == len(bins)
    worst = 0.0
    for k, line in zip(bins, lines):
        kk, re, im = line.split()
        assert int(kk) == k
        re, im = float.fromhex(re), float.fromhex(im)
        assert np.float32(re) == re and np.float32(im) == im  # fp32 values
        wre, wim, turns = _exact_factor(k, n, delta)
        slack = 2 * np.pi * turns * 2.0 ** -52 + 1e-18
        for got, want in ((re, wre), (im, wim)):
            step = float(np.spacing(np.float32(abs(float(want)))))
            err = abs(float(np.longdouble(got) - want))
            worst = max(worst, err / (step + slack))
            assert err <= step + slack, (n, delta, k, got, float(want))
        if 2 * k == n:
            assert im == 0.0                                  # the Nyquist factor is real
    print("MEASURED rotate phases n %d delta %g: worst error %.3g of the allowance" % (n, delta, worst))


def test_zero_shift_gives_exactly_one(phase_driver):
    """theta = 0: a = -0.0, b = 0.0, every delta is a zero and every factor exactly (1, 0), the Nyquist bin included"""
    a, b = (float.fromhex(x) for x in _run(phase_driver, ["coefficients", 0.0])[0].split())
    assert a == 0.0 and b == 0.0
    for n, delta in ((64, 0.0), (64, -0.0), (45, -0.0), (4096, 0.0)):
        for line in _run(phase_driver, [n, delta] + list(range(0, n, max(1, n // 16))) + [n // 2, n - 1]):
            _, re, im = line.split()
            assert float.fromhex(re) == 1.0 and float.fromhex(im) == 0.0, (n, delta, line)


@pytest.mark.parametrize("theta", [0.02, -0.3, 0.7, 1.5, -np.pi / 2])
def test_shear_coefficients(phase_driver, theta):
    a, b = (float.fromhex(x) for x in _run(phase_driver, ["coefficients", float(theta).hex()])[0].split())
    assert abs(a - -np.tan(theta / 2)) <= 2 * np.spacing(abs(a)) and abs(b - np.sin(theta)) <= 2 * np.spacing(abs(b))
    assert abs(a) <= 1.0 and abs(b) <= 1.0                    # |theta| <= pi / 2: no shear moves a line by more than its distance
