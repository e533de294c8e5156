"""ctypes loader of the C-ABI library (include/fftup.h).  No fallback: if libfftup.so is missing or
fails to load, importing the product path raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libfftup.so")

FFTUP_NUM_KERNELS = 4

FLAG_U8_WRAP = 1
FLAG_FUSE_U8_LOAD = 2
FLAG_GENERIC_KERNELS = 4
FLAG_UNFUSED_SHARPEN = 8
FLAG_TUNE_PLAN = 16
FLAG_FUSE_U8_STORE = 32
FLAG_SEQUENTIAL_EXECUTE = 64      # (accepted and ignored: ordered iterations are the default)
FLAG_OVERLAP_ITERATIONS = 128
FLAG_DCT = 256                    # DCT-II -> zero-pad -> DCT-III instead of the periodic FFT (library 0.7.0 on)
FLAG_DOWNSCALE = 512              # upscale in [1/8, 1): spectrum cropped (older libraries refuse such plans: FFTUP_E_INVALID_ARG)
FLAG_ANY_SIZE = 1024              # even lengths with a prime factor above 7, up to 4096: Bluestein transforms (older libraries: FFTUP_E_UNSUPPORTED_SIZE)
FLAG_ODD_SIZE = 2048              # odd widths and heights: exact trigonometric resampling per axis (older libraries: FFTUP_E_INVALID_ARG)
FLAG_MIRROR = 4096                # view plans only: the frame continued by its half-sample even reflection, no wrap at the borders (older libraries ignore the bit)

# fftup_plan_create_size: where the output pixels sit
ALIGN_CORNER = 0                  # output pixel 0 on input pixel 0, as every other FFT plan
ALIGN_CENTRE = 1                  # pixel centres aligned: output pixel m at input position (m + 1/2) N / M - 1/2

# fftup_device_image.format (fftup_execute_device)
FMT_RGB8 = 0                      # interleaved 8-bit RGB, rows of row_stride_bytes
FMT_PLANAR = 1                    # 3 planes in the plan's storage type

# fftup_path_config.mode (fftup_shift_path)
PATH_ABSOLUTE = 0                 # in[i]: frame i against one fixed reference
PATH_CONSECUTIVE = 1              # in[i]: frame i against frame i - 1 (in[0] is ignored)
PATH_MAX_FRAMES = 4096

# every symbol include/fftup.h declares
EXPORTS = [
    "fftup_device_count", "fftup_device_name", "fftup_plan_create", "fftup_plan_destroy", "fftup_plan_info",
    "fftup_upload_rgb8", "fftup_upload_rgb8_slot", "fftup_upload_planar", "fftup_execute", "fftup_execute_ring", "fftup_execute_ring_timed",
    "fftup_profile_kernels", "fftup_download_rgb8", "fftup_download_planar", "fftup_download_presharpen",
    "fftup_download_input_planar", "fftup_host_alloc", "fftup_host_free", "fftup_submit_rgb8", "fftup_wait",
    "fftup_drain", "fftup_strerror", "fftup_last_error", "fftup_version", "fftup_jit_check", "fftup_plan_describe",
    "fftup_device_pci_bus_id", "fftup_output_checksum", "fftup_png_bound", "fftup_submit_png", "fftup_wait_png",
    "fftup_plan_create_size", "fftup_execute_device", "fftup_device_alloc", "fftup_device_free", "fftup_device_copy",
    "fftup_stream_create", "fftup_stream_destroy", "fftup_plan_create_view", "fftup_plan_set_view",
    "fftup_execute_device_views", "fftup_download_view_tables",
    "fftup_align_create", "fftup_align_destroy", "fftup_align_get_info", "fftup_align_shifts",
    "fftup_execute_device_views_shifted", "fftup_shift_path",
    "fftup_rotate_create", "fftup_rotate_destroy", "fftup_rotate_get_info", "fftup_rotate_frames",
    "fftup_roll_create", "fftup_roll_destroy", "fftup_roll_get_info", "fftup_roll_angles", "fftup_rotate_frames_angles",
]
ABI_VERSION = 2


class Config(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32), ("upscale", C.c_float),
                ("precision", C.c_uint32), ("sharpen", C.c_float), ("device", C.c_int32), ("flags", C.c_uint32),
                ("ring", C.c_uint32)]


class Info(C.Structure):
    _fields_ = [("out_width", C.c_uint32), ("out_height", C.c_uint32), ("num_kernels", C.c_uint32),
                ("tuned", C.c_uint32), ("alg_bytes_per_frame", C.c_double),
                ("kernel_alg_bytes", C.c_double * FFTUP_NUM_KERNELS), ("device_bytes", C.c_uint64),
                ("device_name", C.c_char * 256), ("kernel_names", (C.c_char * 64) * FFTUP_NUM_KERNELS),
                # appended in ABI version 2
                ("kernel_min_bytes", C.c_double * FFTUP_NUM_KERNELS), ("abi_version", C.c_uint32), ("u8_store", C.c_uint32)]


class DeviceImageDesc(C.Structure):
    """fftup_device_image"""
    _fields_ = [("data", C.c_void_p), ("format", C.c_uint32), ("row_stride_bytes", C.c_size_t), ("plane_stride_bytes", C.c_size_t)]


class View(C.Structure):
    """fftup_view: the rectangle of the frame a view plan shows, origin and span per axis in input pixels"""
    _fields_ = [("origin_x", C.c_double), ("origin_y", C.c_double), ("span_x", C.c_double), ("span_y", C.c_double)]


class AlignConfig(C.Structure):
    """fftup_align_config"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("precision", C.c_uint32), ("device", C.c_int32),
                ("window_w", C.c_uint32), ("window_h", C.c_uint32), ("decimate", C.c_uint32), ("band", C.c_float),
                ("upsample", C.c_uint32), ("max_batch", C.c_uint32)]


class Shift(C.Structure):
    """fftup_shift: cur(x, y) ~ ref(x - dx, y - dy), in input pixels"""
    _fields_ = [("dx", C.c_float), ("dy", C.c_float), ("peak", C.c_float), ("peak_coarse", C.c_float)]


class AlignInfo(C.Structure):
    """fftup_align_info"""
    _fields_ = [("window_w", C.c_uint32), ("window_h", C.c_uint32), ("decimate", C.c_uint32), ("crop_x", C.c_uint32),
                ("crop_y", C.c_uint32), ("upsample", C.c_uint32), ("band_kx", C.c_uint32), ("band_ky", C.c_uint32),
                ("num_kernels", C.c_uint32), ("device_bytes", C.c_uint64), ("kernel_names", (C.c_char * 64) * 8)]


class PathConfig(C.Structure):
    """fftup_path_config"""
    _fields_ = [("mode", C.c_uint32), ("sigma", C.c_float), ("min_peak", C.c_float)]


class RotateConfig(C.Structure):
    """fftup_rotate_config"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("precision", C.c_uint32), ("device", C.c_int32),
                ("max_batch", C.c_uint32)]


class Rotation(C.Structure):
    """fftup_rotation: content turns by `angle` radians about (centre_x, centre_y), clockwise on screen for a positive angle"""
    _fields_ = [("angle", C.c_double), ("centre_x", C.c_double), ("centre_y", C.c_double)]


class RotateInfo(C.Structure):
    """fftup_rotate_info"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("num_kernels", C.c_uint32), ("max_batch", C.c_uint32),
                ("device_bytes", C.c_uint64), ("kernel_names", (C.c_char * 64) * 4)]


class RollConfig(C.Structure):
    """fftup_roll_config"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("precision", C.c_uint32), ("device", C.c_int32),
                ("window_w", C.c_uint32), ("window_h", C.c_uint32), ("decimate", C.c_uint32), ("band", C.c_float),
                ("angles", C.c_uint32), ("upsample", C.c_uint32), ("max_batch", C.c_uint32)]


class RollAngle(C.Structure):
    """fftup_roll_angle: cur ~ ref turned by `angle` radians, the rotator's sign"""
    _fields_ = [("angle", C.c_float), ("peak", C.c_float), ("peak_coarse", C.c_float), ("reserved", C.c_float)]


class RollInfo(C.Structure):
    """fftup_roll_info"""
    _fields_ = [(k, C.c_uint32) for k in ("window_w", "window_h", "decimate", "crop_x", "crop_y", "upsample", "n", "angles", "rho_min",
                                          "rho_max", "m_band", "K", "max_batch", "num_kernels")] + \
               [("device_bytes", C.c_uint64), ("kernel_names", (C.c_char * 64) * 8)]


KNOBS_LIB_PATH = os.path.join(HERE, "libfftup_knobs.so")       # the same objects + the FFTUP_EXPERIMENT parser (tests, tools)
_libs = {}


def load():
    """Load libfftup.so (built by __graft_entry__.build()).  Raises if it is absent.
    FFTUP_LIBRARY=<path> names another build of the library (tests that pin factorizations or strip lengths through
    FFTUP_EXPERIMENT load libfftup_knobs.so this way: the shipping library has no such parser); read at every call, one
    handle per path."""
    path = os.environ.get("FFTUP_LIBRARY") or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % path)
    lib = C.CDLL(path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.fftup_device_count.restype = C.c_int
    lib.fftup_device_name.argtypes = [C.c_int, C.c_char_p, sz]
    lib.fftup_plan_create.argtypes = [C.POINTER(vp), C.POINTER(Config)]
    lib.fftup_plan_create_size.argtypes = [C.POINTER(vp), C.POINTER(Config), u32, u32, u32]
    lib.fftup_plan_create_view.argtypes = [C.POINTER(vp), C.POINTER(Config), u32, u32, C.POINTER(View)]
    lib.fftup_plan_set_view.argtypes = [vp, C.POINTER(View)]
    lib.fftup_plan_destroy.argtypes = [vp]
    lib.fftup_plan_destroy.restype = None
    lib.fftup_plan_info.argtypes = [vp, C.POINTER(Info)]
    lib.fftup_upload_rgb8.argtypes = [vp, vp, sz]
    lib.fftup_upload_rgb8_slot.argtypes = [vp, u32, vp, sz]
    lib.fftup_upload_planar.argtypes = [vp, u32, vp, sz, sz]
    lib.fftup_execute.argtypes = [vp, u32, C.POINTER(C.c_double)]
    lib.fftup_execute_ring.argtypes = [vp, u32, u32, C.POINTER(C.c_double)]
    lib.fftup_execute_ring_timed.argtypes = [vp, u32, u32, u32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.fftup_profile_kernels.argtypes = [vp, u32, C.POINTER(C.c_double)]
    lib.fftup_download_rgb8.argtypes = [vp, u32, vp, sz]
    lib.fftup_download_planar.argtypes = [vp, u32, vp]
    lib.fftup_download_presharpen.argtypes = [vp, vp]
    lib.fftup_download_input_planar.argtypes = [vp, u32, vp]
    lib.fftup_host_alloc.argtypes = [sz]
    lib.fftup_host_alloc.restype = vp
    lib.fftup_host_free.argtypes = [vp]
    lib.fftup_host_free.restype = None
    lib.fftup_submit_rgb8.argtypes = [vp, vp, sz, vp, sz, C.POINTER(C.c_uint64)]
    lib.fftup_wait.argtypes = [vp, C.c_uint64]
    lib.fftup_drain.argtypes = [vp]
    lib.fftup_png_bound.argtypes = [vp]
    lib.fftup_png_bound.restype = sz
    lib.fftup_submit_png.argtypes = [vp, vp, sz, vp, sz, C.POINTER(C.c_uint64)]
    lib.fftup_wait_png.argtypes = [vp, C.c_uint64, vp, sz, C.POINTER(sz)]
    lib.fftup_strerror.argtypes = [C.c_int]
    lib.fftup_strerror.restype = C.c_char_p
    lib.fftup_last_error.restype = C.c_char_p
    lib.fftup_version.restype = C.c_char_p
    lib.fftup_plan_describe.argtypes = [vp, C.c_char_p, sz]
    lib.fftup_jit_check.argtypes = [u32, u32, C.c_float, u32, C.c_char_p, C.c_char_p, sz]
    lib.fftup_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, sz]
    lib.fftup_output_checksum.argtypes = [vp, u32, C.POINTER(C.c_uint64)]
    lib.fftup_execute_device.argtypes = [vp, C.POINTER(DeviceImageDesc), C.POINTER(DeviceImageDesc), u32, vp]
    lib.fftup_execute_device_views.argtypes = [vp, C.POINTER(DeviceImageDesc), C.POINTER(DeviceImageDesc), C.POINTER(View), u32, vp]
    lib.fftup_download_view_tables.argtypes = [vp, u32, u32, vp, vp, vp, C.POINTER(C.c_int32)]
    lib.fftup_device_alloc.argtypes = [C.c_int, sz]
    lib.fftup_device_alloc.restype = vp
    lib.fftup_device_free.argtypes = [vp]
    lib.fftup_device_free.restype = None
    lib.fftup_device_copy.argtypes = [vp, vp, sz, C.c_int, vp]
    lib.fftup_stream_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.fftup_stream_destroy.argtypes = [vp]
    lib.fftup_align_create.argtypes = [C.POINTER(vp), C.POINTER(AlignConfig)]
    lib.fftup_align_destroy.argtypes = [vp]
    lib.fftup_align_destroy.restype = None
    lib.fftup_align_get_info.argtypes = [vp, C.POINTER(AlignInfo)]
    lib.fftup_align_shifts.argtypes = [vp, C.POINTER(DeviceImageDesc), C.POINTER(DeviceImageDesc), u32, vp, vp]
    lib.fftup_execute_device_views_shifted.argtypes = [vp, C.POINTER(DeviceImageDesc), C.POINTER(DeviceImageDesc), C.POINTER(View), vp, u32, vp]
    lib.fftup_shift_path.argtypes = [C.POINTER(PathConfig), vp, vp, u32, vp]
    lib.fftup_rotate_create.argtypes = [C.POINTER(vp), C.POINTER(RotateConfig)]
    lib.fftup_rotate_destroy.argtypes = [vp]
    lib.fftup_rotate_destroy.restype = None
    lib.fftup_rotate_get_info.argtypes = [vp, C.POINTER(RotateInfo)]
    lib.fftup_rotate_frames.argtypes = [vp, C.POINTER(DeviceImageDesc), C.POINTER(DeviceImageDesc), C.POINTER(Rotation), u32, vp]
    lib.fftup_roll_create.argtypes = [C.POINTER(vp), C.POINTER(RollConfig)]
    lib.fftup_roll_destroy.argtypes = [vp]
    lib.fftup_roll_destroy.restype = None
    lib.fftup_roll_get_info.argtypes = [vp, C.POINTER(RollInfo)]
    lib.fftup_roll_angles.argtypes = [vp, C.POINTER(DeviceImageDesc), C.POINTER(DeviceImageDesc), u32, vp, vp]
    lib.fftup_rotate_frames_angles.argtypes = [vp, C.POINTER(DeviceImageDesc), C.POINTER(DeviceImageDesc), C.POINTER(Rotation), vp, C.c_double, u32, vp]
    _libs[path] = lib
    return lib
