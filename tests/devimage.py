"""Images in caller-owned device memory for the tests of fftup_execute_device, fftup_execute_device_views and fftup_align_shifts:
every image sits in a buffer with 256-byte guard bands in front and behind, pre-filled with 0xA5 like all row and plane padding,
so that a test can tell the pixels from every byte a kernel had no business writing.  Test infrastructure only."""
import numpy as np

GUARD = 256
FILL = 0xA5
RGB8, PLANAR = 0, 1
ESZ = {0: 4, 1: 8, 2: 2}
DTYPE = {0: np.float32, 1: np.float64, 2: np.float16}


def layout(fmt, w, h, esz, padded):
    """(row bytes, row stride, plane stride, planes): dense, or rows padded by 5 bytes (RGB8) / 3 elements (PLANAR) and planes
    by 2 rows"""
    if fmt == RGB8:
        return 3 * w, 3 * w + (5 if padded else 0), 0, 1
    rs = (w + (3 if padded else 0)) * esz
    return w * esz, rs, (h + (2 if padded else 0)) * rs, 3


def _pixel_mask(total, base, planes, plane_stride, rows, row_stride, row_bytes):
    m = np.zeros(total, dtype=bool)
    for c in range(planes):
        for y in range(rows):
            o = base + c * plane_stride + y * row_stride
            m[o:o + row_bytes] = True
    return m


class Image:
    """a device buffer holding one image at `base` bytes from its start, everything else 0xA5"""

    def __init__(self, fmt, w, h, esz, padded=False, base=GUARD, frame=None):
        import vkresample_amd as v
        self.fmt = fmt
        self.row_bytes, self.row_stride, self.plane_stride, self.planes = layout(fmt, w, h, esz, padded)
        extent = self.planes * self.plane_stride if fmt == PLANAR else h * self.row_stride
        self.total = base + extent + GUARD
        self.base = base
        self.mask = _pixel_mask(self.total, base, self.planes, self.plane_stride, h, self.row_stride, self.row_bytes)
        host = np.full(self.total, FILL, dtype=np.uint8)
        if frame is not None:
            host[self.mask] = np.ascontiguousarray(frame).reshape(-1).view(np.uint8)
        self.buf = v.DeviceBuffer(self.total)
        self.buf.upload(host)
        self.image = v.DeviceImage(self.buf.ptr + base, fmt, self.row_stride, self.plane_stride)

    def read(self, stream=None):
        """-> (the pixels' bytes in dense order, True if every other byte is still 0xA5)"""
        got = self.buf.download(stream=stream)
        return got[self.mask], bool((got[~self.mask] == FILL).all())

    def close(self):
        self.buf.close()


def device_run(up, fmt_in, frame, fmt_out, in_padded=False, out_padded=False, in_base=GUARD, out_base=GUARD, stream=None):
    """`frame` through up.execute_device -> Image.read() of the output image"""
    esz = ESZ[up.precision]
    src = Image(fmt_in, up.width, up.height, esz, in_padded, in_base, frame)
    dst = Image(fmt_out, up.out_width, up.out_height, esz, out_padded, out_base)
    try:
        up.execute_device(src.image, dst.image, stream)
        return dst.read(stream)
    finally:
        src.close()
        dst.close()
