"""GPU suite: plans created on the real device say what they said before plan creation was split into the device-free planner
(csrc/plan_rules.hpp) and a device stage -- fftup_plan_describe, the fftup_plan_info names and byte counts, device_bytes -- for
the small rows of tests/golden/plan_geometry.json (every length at most 1024, two shapes specialised at plan time).  This covers
filling the planner's device facts from the real hipDeviceProp_t.  No frame runs."""
import ctypes as C
import json
import os

import pytest

from vkresample_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "plan_geometry.json")) as f:
    _ROWS = [r for r in json.load(f)["rows"] if r["gpu"]]


@pytest.mark.gpu
@pytest.mark.parametrize("row", _ROWS, ids=[r["name"] for r in _ROWS])
def test_plan_reports_as_before_the_split(row):
    lib = _lib.load()
    cfg = _lib.Config(row["width"], row["height"], 3, row["upscale"], row["precision"], 0.2, 0, row["flags"], row["ring"])
    h = C.c_void_p()
    if row["entry"] == "create":
        rc = lib.fftup_plan_create(C.byref(h), C.byref(cfg))
    elif row["entry"] == "size":
        rc = lib.fftup_plan_create_size(C.byref(h), C.byref(cfg), row["out"][0], row["out"][1], row["align"])
    else:
        view = _lib.View(*row["view"])
        rc = lib.fftup_plan_create_view(C.byref(h), C.byref(cfg), row["out"][0], row["out"][1], C.byref(view))
    assert rc == 0, lib.fftup_last_error().decode()
    try:
        buf = C.create_string_buffer(2048)
        assert lib.fftup_plan_describe(h, buf, 2048) == 0
        info = _lib.Info()
        assert lib.fftup_plan_info(h, C.byref(info)) == 0
    finally:
        lib.fftup_plan_destroy(h)
    got = {"out_width": info.out_width, "out_height": info.out_height, "num_kernels": info.num_kernels, "tuned": info.tuned,
           "kernel_names": [bytes(n).split(b"\0")[0].decode() for n in info.kernel_names],
           "alg_bytes_per_frame": info.alg_bytes_per_frame, "kernel_alg_bytes": list(info.kernel_alg_bytes),
           "kernel_min_bytes": list(info.kernel_min_bytes), "u8_store": info.u8_store, "device_bytes": info.device_bytes}
    assert buf.value.decode() == row["describe"]
    assert got == row["info"]
