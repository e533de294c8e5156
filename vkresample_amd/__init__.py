"""vkresample_amd -- MI355X-native FFT upscaler, drop-in for VkResample's upscale path.

Product = vkresample_amd/libfftup.so (hand-written HIP for gfx950 behind the C ABI of include/fftup.h)
plus the C++ CLI (vkresample_amd/csrc/cli).  This package is the thin Python host mirror used by tests
and bench.py.  Nothing here computes on the CPU."""
from .api import Aligner, stabilised_views  # noqa: F401
from .api import Roller, Rotator  # noqa: F401
from .api import PATH_ABSOLUTE, PATH_CONSECUTIVE, PATH_MAX_FRAMES, shift_path  # noqa: F401
from .api import DeviceBuffer, DeviceImage, FftupError, PinnedArray, Stream, Upscaler, device_count, device_name, device_pci_bus_id, upscale_image, view_of_rect, views_between  # noqa: F401
from ._lib import ALIGN_CENTRE, ALIGN_CORNER, FLAG_ANY_SIZE, FLAG_DCT, FLAG_DOWNSCALE, FLAG_FUSE_U8_LOAD, FLAG_FUSE_U8_STORE, FLAG_GENERIC_KERNELS, FLAG_MIRROR, FLAG_ODD_SIZE, FLAG_OVERLAP_ITERATIONS, FLAG_SEQUENTIAL_EXECUTE, FLAG_TUNE_PLAN, FLAG_U8_WRAP, FLAG_UNFUSED_SHARPEN, FMT_PLANAR, FMT_RGB8  # noqa: F401
