"""CPU suite: the device-free planner (csrc/plan_rules.hpp).

Error paths: validation is arithmetic and runs before any device access, so a machine without a GPU answers every invalid request
with the request's own code and text.  tests/golden/plan_errors.json holds what the library answered BEFORE plan creation was
split into plan_check / plan_geometry (one row per rule, all three creation entry points and fftup_plan_set_view(NULL, ..), plus
valid requests whose answer without a device is FFTUP_E_NO_DEVICE); the replay compares code and text exactly.

Decisions: tests/plan_rules_driver.cpp runs plan_check + plan_geometry for the requests of tests/golden/plan_geometry.json with the
device facts recorded there (an MI355X: LDS bytes per workgroup, compute units, architecture name) and prints every PlanGeometry
field; the expected lines are what the library's plans held on that device before the split.  The driver treats a
fftup_jit::choose that succeeds as a specialisation that loaded (on the device it always did), and runs with an empty cache
directory, so that no wisdom file changes a factorization.

Which rows of plan_geometry.json reach what (family; how the column tile width TK was chosen; the rest):
    tuned_*                          tuned; TK 4 of the tuned kernels; fused, u8out (u8store), unfused; ring 4 changes the strip length
    aot_*                            mixed_aot; TK 4 (mixed 1 and 2); fused and unfused
    jit_240x126_u2, jit_96x64_u*,
    jit_1920x1080_u4_3, fourcol_64x8192   mixed_jit; TK 4 of the specialised column kernel (factors 2, 1.5, 1.25, 3 and 4/3)
    jit_96x54_u4_3, generic_64x32_u1.57   generic, no specialisation; TK 8 by the ping-pong rule
    generic_512x256, _1920x1080, _240x126_p2, _64x4096, fourcol_64x8192_generic, any_1366x768
                                     generic, polyphase column (poly) at TK 8, 4, 8, 2, 1, 8
    f64_256x128 / f64_256x128_u1.5   f64; poly / inplaceC; inplaceF and inplaceI (rows in one buffer)
    cplx_8192x64 / _16384x64 / _4096x64_p1 / _32768x16   cplx; inplaceI / inplaceF + fourI / fourI / fourF + fourI
    fourcol_64x16384(_generic)       generic; TK 1, colF and colI (four-step columns)
    dct_64x32, dct_down_64x32, thin_dct_16x256   dct (up, down); ping-pong rule
    down_64x32, thin_down_16x512     down; ping-pong rule
    any_46x22, thin_any_16x262       generic with Bluestein lengths; TK by the Bluestein rule
    odd_63x35, thin_odd_15x243, exact_64x32_100x50_corner / _centre   odd (exact, align 0 / 1); TK by the Bluestein rule
    view_64x32_96x48, thin_view_16x256_32x512   view; TK by the view rule
Not reached by any row: a specialisation that loads for a plan whose size-generic columns would have run in four steps (the reset of
colF / colI in plan_geometry_finish): no such shape has a specialised factorization.  Messages no request can reach, so no row of
plan_errors.json has them: "FFTUP_FLAG_DOWNSCALE: the output sizes must be at least 2 and below the input's" (the even-size rule
answers first, and a factor below 1 always shrinks), "row too long: no four-step split ..." (every 2,3,5,7-smooth length up to
64 x 65536 has a split that fits), and the two messages of fftup_plan_set_view that need a plan (tests/test_gpu_view.py has them)."""
import ctypes as C
import json
import os

import pytest

import plan_driver
from vkresample_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _rows(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def ask(r):
    """(code, fftup_last_error text) of one request of plan_errors.json"""
    lib = _lib.load()
    cfg = _lib.Config(r["width"], r["height"], r["channels"], float(r["upscale"]), r["precision"], float(r["sharpen"]), 0, r["flags"], r["ring"])
    h = C.c_void_p()
    out = None if "out" in r["null"] else C.byref(h)
    cfgp = None if "cfg" in r["null"] else C.byref(cfg)
    view = _lib.View(*[float(x) for x in r["view"]])
    viewp = None if "view" in r["null"] else C.byref(view)
    if r["entry"] == "create":
        code = lib.fftup_plan_create(out, cfgp)
    elif r["entry"] == "size":
        code = lib.fftup_plan_create_size(out, cfgp, r["out"][0], r["out"][1], r["align"])
    elif r["entry"] == "view":
        code = lib.fftup_plan_create_view(out, cfgp, r["out"][0], r["out"][1], viewp)
    else:
        assert r["entry"] == "set_view" and "plan" in r["null"]
        code = lib.fftup_plan_set_view(None, viewp)
    text = lib.fftup_last_error().decode()
    if code == 0:                       # (a machine with a GPU makes the valid requests' plans)
        lib.fftup_plan_destroy(h)
    return code, text


_ERRORS = _rows("plan_errors.json")["rows"]


@pytest.mark.parametrize("row", _ERRORS, ids=[r["name"] for r in _ERRORS])
def test_error_code_and_text_as_before_the_split(row):
    code, text = ask(row)
    if row["code"] == 4 and _lib.load().fftup_device_count() > 0:
        assert code == 0, text          # a valid request: FFTUP_E_NO_DEVICE only where there is none
        return
    assert (code, text) == (row["code"], row["text"])


def test_error_table_reaches_every_rule():
    """one row per message of the validation (the three creation entry points, fftup_plan_set_view(NULL, ..)), each of the four
    bounds of the Bluestein / odd / exact-size plans under each of its three prefixes, and about ten valid requests"""
    texts = {r["text"] for r in _ERRORS}
    # 41 messages a request can reach without a device (two with two lengths in them), and "no HIP device"
    assert len(texts) >= 43
    for prefix in ("FFTUP_FLAG_ANY_SIZE", "FFTUP_FLAG_ODD_SIZE", "fftup_plan_create_size"):
        assert sum(1 for t in texts if prefix in t and ("FFTUP_FLAG_DCT" in t or "-p 0 and -p 2" in t or "8192" in t or "fit the LDS" in t)) >= 4, prefix
    assert sum(1 for r in _ERRORS if r["code"] == 4) >= 10


@pytest.fixture(scope="module")
def driver_lines(tmp_path_factory):
    """the driver, linked from the library's own object files (plan_rules, the kernel facts of fftup_launch, the chooser of jit),
    run once over every request of plan_geometry.json (tests/plan_driver.py)"""
    d = tmp_path_factory.mktemp("plan_rules")
    g = _rows("plan_geometry.json")
    lines = [plan_driver.request_line(r["entry"], r["width"], r["height"], r["upscale"], r["precision"], r["flags"], r["ring"], r["out"], r["align"],
                                      r["view"]) for r in g["rows"]]
    out = plan_driver.run(plan_driver.build(d), d, lines)
    return dict(zip([r["name"] for r in g["rows"]], out))


_GEOMETRY = _rows("plan_geometry.json")["rows"]


@pytest.mark.parametrize("row", _GEOMETRY, ids=[r["name"] for r in _GEOMETRY])
def test_decisions_as_before_the_split(row, driver_lines):
    got, want = driver_lines[row["name"]].split(), row["geometry"].split()
    assert [g for g, w in zip(got, want) if g != w] == [] and len(got) == len(want), "\n%s\n%s" % (driver_lines[row["name"]], row["geometry"])


def test_request_list_reaches_every_branch():
    """every Family value, every way the column tile width is chosen (`TK`), poly, the three in-place variants, each four-step split"""
    f = [dict(kv.split("=", 1) for kv in r["geometry"].split()) for r in _GEOMETRY]
    assert {int(x["family"]) for x in f} == set(range(10))
    for key in ("poly", "inplaceC", "inplaceF", "inplaceI", "tuned", "fused", "u8out", "bz", "odd", "exact", "view", "down", "dct", "cplx", "dbl", "half"):
        assert {x[key] for x in f} == {"0", "1"}, key
    for key in ("fourF", "fourI", "colF", "colI"):
        assert {x[key][0] for x in f} == {"0", "1"}, key
    assert {x["mixed"] for x in f} == {"0", "1", "2", "3"} and {x["TK"] for x in f} >= {"1", "2", "4", "8"}
