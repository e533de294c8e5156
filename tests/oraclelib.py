"""ctypes binding of the CPU oracle (oracle/libfftup_oracle.so).  Test infrastructure only."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
SO = os.path.join(ORACLE_DIR, "libfftup_oracle.so")


class OrcConfig(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("upscale", C.c_float),
                ("precision", C.c_uint32), ("sharpen", C.c_float), ("u8_wrap", C.c_uint32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(ORACLE_DIR, "fftup_oracle.c")
        if not os.path.exists(SO) or os.path.getmtime(SO) < os.path.getmtime(src):
            subprocess.check_call(["make", "-C", ORACLE_DIR, "libfftup_oracle.so"])
        _lib = C.CDLL(SO)
        _lib.orc_load_u8.restype = C.c_double
        _lib.orc_load_u8.argtypes = [C.c_uint32, C.c_uint8]
        _lib.orc_store_u8.restype = C.c_uint8
        _lib.orc_store_u8.argtypes = [C.c_double, C.c_uint32]
    return _lib


def _cfg(W, H, upscale=2.0, precision=0, sharpen=0.2, u8_wrap=0):
    return OrcConfig(W, H, upscale, precision, sharpen, u8_wrap)


def out_dims(W, H, upscale):
    uW, uH = C.c_uint32(), C.c_uint32()
    cfg = _cfg(W, H, upscale)
    lib().orc_out_dims(C.byref(cfg), C.byref(uW), C.byref(uH))
    return uW.value, uH.value


def check(W, H, upscale=2.0, precision=0):
    cfg = _cfg(W, H, upscale, precision)
    return lib().orc_check(C.byref(cfg))


def fft1d(x, sign):
    x = np.ascontiguousarray(x, dtype=np.complex128).copy()
    rc = lib().orc_fft1d(x.ctypes.data_as(C.c_void_p), C.c_uint32(x.size), C.c_int(sign))
    if rc:
        raise ValueError("oracle fft1d rc=%d" % rc)
    return x


def load_lut(precision):
    return np.array([lib().orc_load_u8(precision, v) for v in range(256)])


def upscale_planes(planes, upscale=2.0, precision=0, sharpen=0.2):
    """planes: [3][H][W] float64 -> (pre [3][uH][uW], out [3][uH][uW], poison_reads)"""
    planes = np.ascontiguousarray(planes, dtype=np.float64)
    _, H, W = planes.shape
    cfg = _cfg(W, H, upscale, precision, sharpen)
    uW, uH = out_dims(W, H, upscale)
    _fit_threads(uW * uH)
    pre = np.empty((3, uH, uW))
    out = np.empty((3, uH, uW))
    poison = C.c_uint64(0)
    rc = lib().orc_upscale_planes(C.byref(cfg), planes.ctypes.data_as(C.c_void_p),
                                  pre.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                  C.byref(poison))
    if rc:
        raise ValueError("oracle rc=%d" % rc)
    return pre, out, poison.value


def upscale_planes_complex(planes, upscale=2.0, precision=0, sharpen=0.2):
    """the non-R2C path (the reference takes it for uW > 8192; callable at any size here):
    planes [3][H][W] float64 -> (complex pre-sharpen image [3][uH][uW], out [3][uH][uW], poison_reads)"""
    planes = np.ascontiguousarray(planes, dtype=np.float64)
    _, H, W = planes.shape
    cfg = _cfg(W, H, upscale, precision, sharpen)
    uW, uH = out_dims(W, H, upscale)
    _fit_threads(uW * uH)
    re, im, out = np.empty((3, uH, uW)), np.empty((3, uH, uW)), np.empty((3, uH, uW))
    poison = C.c_uint64(0)
    rc = lib().orc_upscale_planes_complex(C.byref(cfg), planes.ctypes.data_as(C.c_void_p), re.ctypes.data_as(C.c_void_p),
                                          im.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(poison))
    if rc:
        raise ValueError("oracle rc=%d" % rc)
    return re + 1j * im, out, poison.value


def uses_complex_path(W, H, upscale=2.0, precision=0):
    cfg = _cfg(W, H, upscale, precision)
    return bool(lib().orc_uses_complex_path(C.byref(cfg)))


def upscale_rgb8(rgb, upscale=2.0, precision=0, sharpen=0.2, u8_wrap=0):
    """rgb: [H][W][3] uint8 -> (pre, out, rgb_out[uH][uW][3])"""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    H, W, _ = rgb.shape
    cfg = _cfg(W, H, upscale, precision, sharpen, u8_wrap)
    uW, uH = out_dims(W, H, upscale)
    _fit_threads(uW * uH)
    pre = np.empty((3, uH, uW))
    out = np.empty((3, uH, uW))
    rgb_out = np.empty((uH, uW, 3), dtype=np.uint8)
    rc = lib().orc_upscale_rgb8(C.byref(cfg), rgb.ctypes.data_as(C.c_void_p),
                                pre.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                rgb_out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError("oracle rc=%d" % rc)
    return pre, out, rgb_out


def presharpen_rgb8(rgb, upscale=2.0, precision=0):
    """rgb: [H][W][3] uint8 -> the pre-sharpen image alone (no sharpen pass: at -p 2 the oracle's binary16 sharpen is the slow part)"""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    H, W, _ = rgb.shape
    cfg = _cfg(W, H, upscale, precision)
    uW, uH = out_dims(W, H, upscale)
    _fit_threads(uW * uH)
    pre = np.empty((3, uH, uW))
    rc = lib().orc_upscale_rgb8(C.byref(cfg), rgb.ctypes.data_as(C.c_void_p), pre.ctypes.data_as(C.c_void_p), None, None)
    if rc:
        raise ValueError("oracle rc=%d" % rc)
    return pre


def sharpen(R, upscale=2.0, precision=0, sharpen=0.2):
    R = np.ascontiguousarray(R, dtype=np.float64)
    _, uH, uW = R.shape
    cfg = _cfg(0, 0, upscale, precision, sharpen)
    out = np.empty_like(R)
    lib().orc_sharpen(C.byref(cfg), R.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                      C.c_uint32(uW), C.c_uint32(uH))
    return out


def sharpen_complex(z, upscale=2.0, precision=0, sharpen=0.2):
    """the filter of the non-R2C path on a complex image z [3][uH][uW]: its taps are |u^2 z|"""
    re, im = np.ascontiguousarray(z.real, dtype=np.float64), np.ascontiguousarray(z.imag, dtype=np.float64)
    _, uH, uW = re.shape
    cfg = _cfg(0, 0, upscale, precision, sharpen)
    out = np.empty_like(re)
    lib().orc_sharpen_complex(C.byref(cfg), re.ctypes.data_as(C.c_void_p), im.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                              C.c_uint32(uW), C.c_uint32(uH))
    return out


_MAX_THREADS = None


def cpu_quota():
    """CPUs' worth of time the container may use (cgroup v2 cpu.max / v1 cfs quota), None without a limit"""
    try:
        if os.path.exists("/sys/fs/cgroup/cpu.max"):
            q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
            return None if q == "max" else float(q) / float(p)
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / p
    except (OSError, ValueError):
        return None


def _fit_threads(pixels):
    """a thread team sized to the image: one thread per ~64k output pixels, at most what the host offers -- the CPUs the
    process may run on and the container's CPU quota (a team of 128 on a 16-CPU quota spends its time in throttled barriers)"""
    global _MAX_THREADS
    L = lib()
    if _MAX_THREADS is None:
        _MAX_THREADS = min(L.orc_num_threads(), len(os.sched_getaffinity(0)))
        q = cpu_quota()
        if q is not None:
            _MAX_THREADS = max(1, min(_MAX_THREADS, int(math.ceil(q))))
    L.orc_set_num_threads(int(min(_MAX_THREADS, max(1, pixels // 65536))))


def num_threads():
    return lib().orc_num_threads()


def readme_panel_mask():
    """Which pixels of a 300x300 FFT panel of the README's comparison strips (tests/golden/readme_*.npz) are compared with
    this code's output: everything but a 12-pixel border (the input beyond the window is known to ~2 grey levels only) and
    the top-right corner, rows < 82 / columns >= 178 -- the panel's own label plus the 12-pixel surroundings of the region
    where the NN panel's label hides the input.  68 476 of 90 000 pixels (round 2 compared a 180x160 box: 28 800)."""
    import numpy as np
    m = np.zeros((300, 300), bool)
    m[12:288, 12:288] = True
    m[:82, 178:] = False
    return m


def readme_panel_stats(u8, d):
    """|code - reference's own pixel| over readme_panel_mask(): mean, p99, p99.9, max, histogram (grey levels 0..7+)"""
    import numpy as np
    Yo, Xo = int(d["Yo"]), int(d["Xo"])
    diff = np.abs(u8[Yo:Yo + 300, Xo:Xo + 300].astype(np.int64) - d["fft_panel"].astype(np.int64))[readme_panel_mask()]
    hist = np.bincount(np.minimum(diff.ravel(), 7), minlength=8)
    return {"mean": float(diff.mean()), "p99": float(np.percentile(diff, 99)), "p99.9": float(np.percentile(diff, 99.9)),
            "max": int(diff.max()), "hist": hist.tolist(), "n": int(diff.size)}
