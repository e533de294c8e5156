"""CPU: fftup_plan_create_view / fftup_plan_set_view are declared in the header, exported and bound; the plan validation is
arithmetic that happens before any device access -- every case below returns the same code with or without a GPU; and the host
tables of the chirp-z transforms (csrc/view_tables.hpp) agree with a longdouble numpy evaluation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import view_oracle as V
from family_sweep_cases import smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (W, H, uW, uH, origin, span, extra flags): the GPU tests' cases, the workload-sized 2x zoom, and the largest row convolution
# (4096 -> 4096: L is exactly 8192)
VALID = [(48, 40, 40, 36, (10.3, 7.75), (17.9, 12.2), ""), (45, 21, 64, 30, (-3.25, 2.5), (61.5, 33.3), ""),
         (50, 32, 32, 20, (5.5, 0.0), (77.7, 40.0), ""), (46, 22, 70, 30, (0.4, 0.6), (23.0, 11.0), "any"),
         (50, 32, 33, 47, (0.0, 0.0), (50.0, 32.0), ""),                 # output lengths with prime factors above 7: no flag needed
         (1920, 1080, 1920, 1080, (480.0, 270.0), (960.0, 540.0), ""), (4096, 8, 4096, 8, (0.5, 0.0), (4096.0, 8.0), ""),
         (64, 48, 64, 48, (1e9, -1e9), (1.0, 384.0), "")]               # steps 1/64 and 8: the bounds are closed


def _flags(v, extra):
    return v.FLAG_ANY_SIZE if "any" in extra else 0


def test_symbols_in_header_library_and_binding():
    import vkresample_amd as v
    from vkresample_amd import _lib
    src = open(os.path.join(ROOT, "include", "fftup.h")).read()
    assert re.search(r"typedef struct fftup_view \{ double origin_x, origin_y, span_x, span_y; \} fftup_view;", src)
    assert re.search(r"FFTUP_API int fftup_plan_create_view\(fftup_plan\*\* out, const fftup_config\* cfg,\s*uint32_t out_width, uint32_t out_height, const fftup_view\* view\);", src)
    assert re.search(r"FFTUP_API int fftup_plan_set_view\(fftup_plan\* plan, const fftup_view\* view\);", src)
    assert "fftup_plan_create_view" in _lib.EXPORTS and "fftup_plan_set_view" in _lib.EXPORTS
    lib = _lib.load()
    assert len(lib.fftup_plan_create_view.argtypes) == 5 and len(lib.fftup_plan_set_view.argtypes) == 2
    assert C.sizeof(_lib.View) == 32 and [f[0] for f in _lib.View._fields_] == ["origin_x", "origin_y", "span_x", "span_y"]
    # the ABI and the version string are the ones before these calls existed: callers detect them by the symbol
    assert re.search(r"\bFFTUP_ABI_VERSION\s*=\s*2\b", src) and lib.fftup_version().decode() == "fftup 0.7.0 (gfx950, ABI 2)"
    assert isinstance(v.Upscaler.__dict__["view"], classmethod) and callable(v.Upscaler.set_view)
    # a rectangle in pixel-edge coordinates, centres aligned: the whole frame is the exact-size plans' centre alignment
    (ox, oy), (sx, sy) = v.view_of_rect(0, 0, 50, 32, 32, 50)
    assert (sx, sy) == (50.0, 32.0) and ox == (50 / 32 - 1) / 2 and oy == (32 / 50 - 1) / 2
    assert v.view_of_rect(480, 270, 960, 540, 1920, 1080) == ((480 - 0.25, 270 - 0.25), (960.0, 540.0))


@pytest.mark.parametrize("W,H,uW,uH,origin,span,extra", VALID)
def test_valid_plans_pass_validation(W, H, uW, uH, origin, span, extra):
    """FFTUP_E_NO_DEVICE on a box without a GPU: everything decided by arithmetic has passed.  FLAG_ODD_SIZE and FLAG_DOWNSCALE are
    implied: accepted, and (sizes, names) stay what they are"""
    import vkresample_amd as v
    seen = []
    for precision in (0, 2):
        for more in (0, v.FLAG_ODD_SIZE | v.FLAG_DOWNSCALE):
            try:
                with v.Upscaler.view(W, H, uW, uH, origin, span, precision, 0.2, 0, _flags(v, extra) | more) as up:
                    assert (up.width, up.height, up.out_width, up.out_height) == (W, H, uW, uH)
                    seen.append((up.kernel_names, up.num_kernels, up.tuned, up.u8_store))
            except v.FftupError as e:
                assert e.code == 4 and v.device_count() == 0, str(e)
    assert all(s == (seen[0][0], 4, False, False) for s in seen)


NAN, INF = float("nan"), float("inf")
INVALID = [
    # (kwargs of Upscaler.view, code, a word of fftup_last_error)
    (dict(width=1, height=32, out_width=2, out_height=32, origin=(0, 0), span=(1, 32)), 1, "at least 2"),
    (dict(width=50, height=1, out_width=50, out_height=2, origin=(0, 0), span=(50, 1)), 1, "at least 2"),
    (dict(width=50, height=32, out_width=1, out_height=32, origin=(0, 0), span=(1, 32)), 1, "at least 2"),
    (dict(width=50, height=32, out_width=50, out_height=0, origin=(0, 0), span=(50, 32)), 1, "at least 2"),
    (dict(width=50, height=32, out_width=32, out_height=50, origin=(NAN, 0), span=(50, 32)), 1, "finite"),
    (dict(width=50, height=32, out_width=32, out_height=50, origin=(0, INF), span=(50, 32)), 1, "finite"),
    (dict(width=50, height=32, out_width=32, out_height=50, origin=(0, 0), span=(NAN, 32)), 1, "finite"),
    (dict(width=50, height=32, out_width=32, out_height=50, origin=(0, 0), span=(50, -INF)), 1, "finite"),
    (dict(width=50, height=32, out_width=32, out_height=50, origin=(0, 0), span=(256.1, 32)), 1, "span_x"),       # step above 8
    (dict(width=50, height=32, out_width=64, out_height=50, origin=(0, 0), span=(0.99, 32)), 1, "span_x"),        # step below 1/64
    (dict(width=50, height=32, out_width=32, out_height=50, origin=(0, 0), span=(50, 400.5)), 1, "span_y"),
    (dict(width=50, height=32, out_width=32, out_height=64, origin=(0, 0), span=(50, 0.5)), 1, "span_y"),
    (dict(width=50, height=32, out_width=32, out_height=50, origin=(0, 0), span=(-50, 32)), 1, "span_x"),         # a negative span
    (dict(width=50, height=32, out_width=32, out_height=50, origin=(0, 0), span=(50, 0)), 1, "span_y"),
    (dict(width=50, height=32, out_width=32, out_height=50, origin=(0, 0), span=(50, 32), precision=1), 3, "-p 0 and -p 2"),
    (dict(width=50, height=32, out_width=32, out_height=50, origin=(0, 0), span=(50, 32), precision=3), 3, "precision"),
    (dict(width=50, height=32, out_width=32, out_height=50, origin=(0, 0), span=(50, 32), flags=256), 2, "FFTUP_FLAG_DCT"),
    (dict(width=8400, height=8, out_width=64, out_height=8, origin=(0, 0), span=(512, 8)), 2, "8192"),           # W above 8192
    (dict(width=46, height=22, out_width=70, out_height=30, origin=(0, 0), span=(46, 22)), 2, "FFTUP_FLAG_ANY_SIZE"),   # 46 = 2 * 23
    (dict(width=64, height=22, out_width=64, out_height=22, origin=(0, 0), span=(64, 22)), 2, "FFTUP_FLAG_ANY_SIZE"),   # the height
    (dict(width=64, height=4098, out_width=64, out_height=64, origin=(0, 0), span=(64, 64), flags=1024), 2, "4096"),    # 4098 = 2 * 3 * 683
    (dict(width=4100, height=8, out_width=4100, out_height=8, origin=(0, 0), span=(4100, 8), flags=1024), 2, "convolution"),  # L would exceed 8192
    (dict(width=4200, height=8, out_width=4000, out_height=8, origin=(0, 0), span=(4200, 8)), 2, "convolution"),        # 4200 + 4000 = 8200
    (dict(width=4096, height=8, out_width=4097, out_height=8, origin=(0, 0), span=(4096, 8)), 2, "convolution"),
    (dict(width=64, height=8192, out_width=64, out_height=2048, origin=(0, 0), span=(64, 8192)), 2, "columns"),   # L_y = 10240: two buffers do not fit
]


@pytest.mark.parametrize("kwargs,code,word", INVALID)
def test_invalid_plans_fail_before_device_access(kwargs, code, word):
    import vkresample_amd as v
    with pytest.raises(v.FftupError) as e:
        v.Upscaler.view(**kwargs)
    assert e.value.code == code, (kwargs, str(e.value))
    assert word in str(e.value), str(e.value)


def test_c_abi_null_pointers_channels_and_set_view():
    from vkresample_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.Config(50, 32, 3, float("nan"), 0, 0.2, 0, 0, 1)        # upscale: ignored by this call
    vw = _lib.View(5.5, 0.0, 77.7, 40.0)
    assert lib.fftup_plan_create_view(None, C.byref(cfg), 32, 20, C.byref(vw)) == 1
    assert lib.fftup_plan_create_view(C.byref(h), None, 32, 20, C.byref(vw)) == 1
    assert lib.fftup_plan_create_view(C.byref(h), C.byref(cfg), 32, 20, None) == 1 and not h.value
    assert b"null" in lib.fftup_last_error()
    for ch in (0, 1, 4):
        cfg.channels = ch
        assert lib.fftup_plan_create_view(C.byref(h), C.byref(cfg), 32, 20, C.byref(vw)) == 1 and not h.value
        assert b"channels" in lib.fftup_last_error()
    cfg.channels = 3
    rc = lib.fftup_plan_create_view(C.byref(h), C.byref(cfg), 32, 20, C.byref(vw))
    assert rc in (0, 4)
    if rc == 0:
        lib.fftup_plan_destroy(h)
    assert lib.fftup_plan_set_view(None, C.byref(vw)) == 1 and b"null" in lib.fftup_last_error()


@pytest.fixture(scope="module")
def tables_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("view") / "view_tables_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "vkresample_amd", "csrc"),
                           os.path.join(ROOT, "tests", "view", "view_tables_driver.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("N,M,origin,span", [(48, 40, 10.3, 17.9), (45, 64, -3.25, 61.5), (50, 32, 5.5, 77.7), (46, 70, 0.4, 23.0),
                                             (4096, 4096, 0.5, 4096.0), (1920, 1920, 480.0 + 1e6 * 1920, 960.0), (1080, 1080, -0.25, 8640.0)])
def test_host_tables_against_longdouble_numpy(tables_driver, N, M, origin, span):
    """kmax and L by the header's rules; every table entry within one fp32 rounding of the longdouble value (phases of tens of
    thousands of radians: formed in fp32, or in double without the reduction, they would be off by 1e-3 and more); bhat against the
    FFT of the wrapped chirp"""
    out = subprocess.run([tables_driver, str(N), str(M), repr(origin), repr(span)], capture_output=True, text=True, check=True).stdout.split("\n")
    kmax, L = (int(t) for t in out[0].split())
    vals = np.array([[float(t) for t in line.split()] for line in out[1:] if line])
    K = 2 * kmax + 1
    assert vals.shape == (K + M + L, 2)
    cplx = vals[:, 0] + 1j * vals[:, 1]
    pre, post, bhat = cplx[:K], cplx[K:K + M], cplx[K + M:]
    k, opre, opost, oc = V.chirp_tables(N, M, origin, span)
    assert kmax == k == V.kmax(N, M, span)
    need = 2 * (N // 2) + M
    assert L >= need and smooth(L) and not any(smooth(q) for q in range(need, L))      # the smallest smooth length that fits
    eps = 2.0 ** -24
    assert np.abs(pre - opre.astype(np.complex128)).max() <= 1.01 * eps
    scale = float(span) / M / N
    assert np.abs(post - opost.astype(np.complex128)).max() <= 1.01 * eps * scale
    cw = np.zeros(L, np.complex128)
    d = np.arange(-(K - 1), M)
    cw[d % L] = oc.astype(np.complex128)
    ref = np.fft.ifft(cw)                                               # FFT with exp(+...) / L
    assert np.abs(bhat - ref).max() <= 1.01 * eps * max(np.abs(ref).max(), 1e-30) + 1e-12
