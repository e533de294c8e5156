"""CPU: fftup_execute_device, fftup_device_image and the device / stream helpers are declared in the header, exported and bound;
their argument checks and their behaviour on a box without a device need no GPU."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_EXPORTS = ["fftup_execute_device", "fftup_device_alloc", "fftup_device_free", "fftup_device_copy", "fftup_stream_create",
               "fftup_stream_destroy"]

SNIPPET = r'''
#include "fftup.h"
int main(void)
{
    fftup_device_image in, out;
    void* s = 0;
    void* p;
    int rc;
    in.data = 0; in.format = FFTUP_FMT_RGB8; in.row_stride_bytes = 3 * 64; in.plane_stride_bytes = 0;
    out.data = 0; out.format = FFTUP_FMT_PLANAR; out.row_stride_bytes = 128 * sizeof(float); out.plane_stride_bytes = 64 * out.row_stride_bytes;
    rc = fftup_execute_device((fftup_plan*)0, &in, &out, 1, s);
    p = fftup_device_alloc(0, 64);
    if (p) { rc += fftup_device_copy(p, p, 0, 2, s); fftup_device_free(p); }
    if (fftup_stream_create(0, &s) == FFTUP_OK) rc += fftup_stream_destroy(s);
    return rc == FFTUP_E_INVALID_ARG ? 0 : 1;
}
'''


def test_header_with_the_new_symbols_compiles_as_c_and_cxx(tmp_path):
    for comp, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        f = tmp_path / ("t." + ext)
        f.write_text(SNIPPET)
        subprocess.check_call([comp, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(f),
                               "-o", str(tmp_path / ("t_" + ext + ".o"))])


def test_descriptor_layout_matches_header(tmp_path):
    """the ctypes mirror of fftup_device_image has the compiler's size and offsets"""
    from vkresample_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fftup.h"\nint main(void){ printf("%zu %zu %zu %zu %zu %d %d\\n", '
                    'sizeof(fftup_device_image), offsetof(fftup_device_image, data), offsetof(fftup_device_image, format), '
                    'offsetof(fftup_device_image, row_stride_bytes), offsetof(fftup_device_image, plane_stride_bytes), '
                    '(int)FFTUP_FMT_RGB8, (int)FFTUP_FMT_PLANAR); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    D = _lib.DeviceImageDesc
    assert got == [C.sizeof(D), D.data.offset, D.format.offset, D.row_stride_bytes.offset, D.plane_stride_bytes.offset,
                   _lib.FMT_RGB8, _lib.FMT_PLANAR]


def test_binding_declares_argtypes_for_every_new_export():
    import vkresample_amd as v
    from vkresample_amd import _lib
    lib = _lib.load()
    want = {"fftup_execute_device": 5, "fftup_device_alloc": 2, "fftup_device_free": 1, "fftup_device_copy": 5,
            "fftup_stream_create": 2, "fftup_stream_destroy": 1}
    assert sorted(want) == sorted(NEW_EXPORTS)
    for name, n in want.items():
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
    assert lib.fftup_device_alloc.restype is C.c_void_p and lib.fftup_device_free.restype is None
    assert (v.FMT_RGB8, v.FMT_PLANAR) == (0, 1)
    for cls in ("DeviceImage", "DeviceBuffer", "Stream"):
        assert isinstance(getattr(v, cls), type)
    assert callable(v.Upscaler.execute_device)
    # callers detect the feature by the symbol: the version string and the ABI number are the ones before it
    assert lib.fftup_version().decode() == "fftup 0.7.0 (gfx950, ABI 2)"


def test_null_plan_is_refused():
    from vkresample_amd import _lib
    lib = _lib.load()
    d = _lib.DeviceImageDesc(None, 0, 0, 0)
    assert lib.fftup_execute_device(None, C.byref(d), C.byref(d), 1, None) == 1
    assert "null" in lib.fftup_last_error().decode()


def test_helpers_without_a_device():
    """no HIP device: the allocator returns NULL with a message, the stream constructor FFTUP_E_NO_DEVICE or FFTUP_E_HIP"""
    import pytest
    import vkresample_amd as v
    from vkresample_amd import _lib
    if v.device_count() > 0:
        pytest.skip("this box has a HIP device")
    lib = _lib.load()
    assert lib.fftup_device_alloc(0, 64) is None
    assert lib.fftup_last_error().decode()
    s = C.c_void_p()
    assert lib.fftup_stream_create(0, C.byref(s)) in (4, 5) and not s.value
    assert lib.fftup_last_error().decode()
    with pytest.raises(v.FftupError):
        v.DeviceBuffer(64)
    with pytest.raises(v.FftupError):
        v.Stream()
