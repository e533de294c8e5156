"""Host-side mirror of the reference's per-image pipeline surface, on top of the C ABI.

Reference (VkResample.cpp): launchResample() VR:1280-1780 builds the plan and runs, per file,
pack+upload (VR:1636-1688) -> performVulkanUpscale(numIter) (VR:1249-1279, VR:1692) -> download+unpack
(VR:1697-1748).  `Upscaler` keeps those three steps and their argument meaning (`upscale`, `precision`,
`sharpen`, `num_iter` = -u/-p/-s/-n).  All compute happens in libfftup.so (HIP); there is no CPU path.
"""
import ctypes as C

import numpy as np

from . import _lib


class FftupError(RuntimeError):
    def __init__(self, code, where):
        lib = _lib.load()
        self.code = code
        detail = lib.fftup_last_error().decode(errors="replace")
        super().__init__("%s failed: %s (%d)%s" % (where, lib.fftup_strerror(code).decode(), code,
                                                   ": " + detail if detail else ""))


def _check(code, where):
    if code != 0:
        raise FftupError(code, where)


def device_count():
    return _lib.load().fftup_device_count()


def device_name(device=0):
    buf = C.create_string_buffer(256)
    _check(_lib.load().fftup_device_name(device, buf, 256), "fftup_device_name")
    return buf.value.decode()


def device_pci_bus_id(device=0):
    buf = C.create_string_buffer(64)
    _check(_lib.load().fftup_device_pci_bus_id(device, buf, 64), "fftup_device_pci_bus_id")
    return buf.value.decode()


class Upscaler:
    """One plan = one (width, height, upscale, precision, sharpen, device) configuration.  `flags`: the FLAG_* bits of _lib
    (include/fftup.h), e.g. FLAG_ANY_SIZE (1024) for even sizes that do not factor into 2,3,5,7, FLAG_ODD_SIZE (2048) for odd widths
    and heights."""

    def __init__(self, width, height, upscale=2.0, precision=0, sharpen=0.2, device=0, flags=0, ring=1):
        self._create(width, height, upscale, precision, sharpen, device, flags, ring, None)

    @classmethod
    def to_size(cls, width, height, out_width, out_height, precision=0, sharpen=0.2, device=0, flags=0, ring=1, align=0):
        """A plan for an exact output size (fftup_plan_create_size): one factor per axis, each axis up, down or equal on its own,
        exact trigonometric resampling on both.  `align`: ALIGN_CORNER (0, output pixel 0 on input pixel 0) or ALIGN_CENTRE (1, pixel
        centres aligned, as OpenCV and PIL place them).  FLAG_ANY_SIZE is still needed for a length with a prime factor above 7."""
        self = cls.__new__(cls)
        self._create(width, height, 1.0, precision, sharpen, device, flags, ring, (out_width, out_height, align))
        return self

    @classmethod
    def view(cls, width, height, out_width, out_height, origin, span, precision=0, sharpen=0.2, device=0, flags=0, ring=1):
        """A view plan (fftup_plan_create_view): the out_width x out_height output shows the rectangle of the frame that starts at
        input position origin = (x, y) and is span = (w, h) input pixels wide and high -- output pixel m of an axis at origin + m span / M,
        any real numbers (zoom, sub-pixel pan, any ratio; the frame is periodic).  view_of_rect gives (origin, span) of a rectangle in
        pixel-edge coordinates.  set_view re-aims the plan.  flags=FLAG_MIRROR: the frame is continued by its half-sample even
        reflection instead of periodically -- a view at a border does not mix in the opposite border (kernel names carry "_mirror")."""
        self = cls.__new__(cls)
        self._create(width, height, 1.0, precision, sharpen, device, flags, ring, (out_width, out_height), (origin, span))
        return self

    def set_view(self, origin, span):
        """Re-aim a view plan (fftup_plan_set_view): blocking, no plan creation; frames executed afterwards show the new view."""
        v = _lib.View(origin[0], origin[1], span[0], span[1])
        _check(self._lib.fftup_plan_set_view(self._h, C.byref(v)), "fftup_plan_set_view")
        buf = C.create_string_buffer(512)
        _check(self._lib.fftup_plan_describe(self._h, buf, 512), "fftup_plan_describe")
        self.description = buf.value.decode()
        info = _lib.Info()
        _check(self._lib.fftup_plan_info(self._h, C.byref(info)), "fftup_plan_info")
        self.alg_bytes_per_frame = info.alg_bytes_per_frame
        self.kernel_alg_bytes = list(info.kernel_alg_bytes)
        self.kernel_min_bytes = list(info.kernel_min_bytes)

    def _create(self, width, height, upscale, precision, sharpen, device, flags, ring, size, view=None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        cfg = _lib.Config(width, height, 3, upscale, precision, sharpen, device, flags, ring)
        if view is not None:
            v = _lib.View(view[0][0], view[0][1], view[1][0], view[1][1])
            _check(self._lib.fftup_plan_create_view(C.byref(self._h), C.byref(cfg), size[0], size[1], C.byref(v)), "fftup_plan_create_view")
        elif size is None:
            _check(self._lib.fftup_plan_create(C.byref(self._h), C.byref(cfg)), "fftup_plan_create")
        else:
            _check(self._lib.fftup_plan_create_size(C.byref(self._h), C.byref(cfg), size[0], size[1], size[2]), "fftup_plan_create_size")
        info = _lib.Info()
        _check(self._lib.fftup_plan_info(self._h, C.byref(info)), "fftup_plan_info")
        if info.abi_version != _lib.ABI_VERSION:
            self._lib.fftup_plan_destroy(self._h)
            self._h = None
            raise RuntimeError("libfftup.so speaks ABI version %d, this binding %d: rebuild (python -c 'import __graft_entry__ as g; g.build()')"
                               % (info.abi_version, _lib.ABI_VERSION))
        self.width, self.height = width, height
        self.out_width, self.out_height = info.out_width, info.out_height
        self.precision = precision
        self.flags = flags
        self.ring = max(1, ring)
        self.alg_bytes_per_frame = info.alg_bytes_per_frame
        self.kernel_alg_bytes = list(info.kernel_alg_bytes)
        self.kernel_min_bytes = list(info.kernel_min_bytes)
        self.kernel_names = [bytes(n).split(b"\0")[0].decode() for n in info.kernel_names]
        self.num_kernels = info.num_kernels
        self.device_name = info.device_name.decode()
        self.device_bytes = info.device_bytes
        self.tuned = bool(info.tuned)
        self.u8_store = bool(info.u8_store)             # output slots hold 8-bit RGB (FLAG_FUSE_U8_STORE in effect)
        _buf = C.create_string_buffer(512)
        _check(self._lib.fftup_plan_describe(self._h, _buf, 512), "fftup_plan_describe")
        self.description = _buf.value.decode()
        self.specialised_at_plan_time = info.tuned == 2      # kernels instantiated for this size through hipRTC (csrc/jit.hpp)
        self._dtype = {0: np.float32, 1: np.float64, 2: np.float16}[precision]

    def close(self):
        if self._h:
            self._lib.fftup_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- pack + transferDataFromCPU (VR:1636-1688)
    def upload_rgb8(self, rgb, slot=0):
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        assert rgb.shape == (self.height, self.width, 3), rgb.shape
        _check(self._lib.fftup_upload_rgb8_slot(self._h, slot, rgb.ctypes.data, rgb.strides[0]), "fftup_upload_rgb8")

    def upload_planar(self, planes, slot=0):
        planes = np.ascontiguousarray(planes, dtype=self._dtype)
        assert planes.shape == (3, self.height, self.width), planes.shape
        _check(self._lib.fftup_upload_planar(self._h, slot, planes.ctypes.data, self.width, self.width * self.height),
               "fftup_upload_planar")

    # ---- performVulkanUpscale (VR:1249-1279): returns ms per iteration
    def execute(self, num_iter=1):
        ms = C.c_double()
        _check(self._lib.fftup_execute(self._h, num_iter, C.byref(ms)), "fftup_execute")
        return ms.value

    def execute_ring(self, n_frames, first_slot=0):
        ms = C.c_double()
        _check(self._lib.fftup_execute_ring(self._h, n_frames, first_slot, C.byref(ms)), "fftup_execute_ring")
        return ms.value

    def execute_ring_timed(self, n_frames, first_slot=0, stride=1):
        """-> (total ms, [ms per kernel]); events around every launch of every stride-th frame, on the launching stream"""
        ms = C.c_double()
        km = (C.c_double * _lib.FFTUP_NUM_KERNELS)()
        _check(self._lib.fftup_execute_ring_timed(self._h, n_frames, first_slot, stride, C.byref(ms), km),
               "fftup_execute_ring_timed")
        return ms.value, list(km)

    def profile_kernels(self, num_iter=10):
        ms = (C.c_double * _lib.FFTUP_NUM_KERNELS)()
        _check(self._lib.fftup_profile_kernels(self._h, num_iter, ms), "fftup_profile_kernels")
        return list(ms)

    # ---- transferDataToCPU + unpack (VR:1697-1748)
    def download_planar(self, slot=0):
        out = np.empty((3, self.out_height, self.out_width), dtype=self._dtype)
        _check(self._lib.fftup_download_planar(self._h, slot, out.ctypes.data), "fftup_download_planar")
        return out

    def download_presharpen(self):
        out = np.empty((3, self.out_height, self.out_width), dtype=self._dtype)
        _check(self._lib.fftup_download_presharpen(self._h, out.ctypes.data), "fftup_download_presharpen")
        return out

    def download_input_planar(self, slot=0):
        out = np.empty((3, self.height, self.width), dtype=self._dtype)
        _check(self._lib.fftup_download_input_planar(self._h, slot, out.ctypes.data), "fftup_download_input_planar")
        return out

    def submit_rgb8(self, rgb_in, rgb_out):
        """Enqueue one host frame end to end (H2D, convert, kernels, convert, D2H) and return its ticket; up to
        `ring` frames are in flight.  rgb_in [H][W][3] / rgb_out [uH][uW][3] uint8, C-contiguous, and they must
        stay alive and untouched until wait(ticket) returns (pinned memory: PinnedArray).  submit_rgb8 / wait / drain of
        one Upscaler may be called from several threads at once (tickets are global to the plan)."""
        assert rgb_in.dtype == np.uint8 and rgb_in.shape == (self.height, self.width, 3) and rgb_in.flags.c_contiguous
        assert rgb_out.dtype == np.uint8 and rgb_out.shape == (self.out_height, self.out_width, 3) and rgb_out.flags.c_contiguous
        t = C.c_uint64()
        _check(self._lib.fftup_submit_rgb8(self._h, rgb_in.ctypes.data, 3 * self.width, rgb_out.ctypes.data,
                                           3 * self.out_width, C.byref(t)), "fftup_submit_rgb8")
        return t.value

    def png_bound(self):
        """bytes a PNG buffer of wait_png needs"""
        return int(self._lib.fftup_png_bound(self._h))

    def submit_png(self, rgb_in, png_out=None):
        """Like submit_rgb8, but the frame is PNG-encoded on the device; collect it with wait_png(ticket, buffer).  With png_out
        (a PinnedArray's uint8 array of png_bound() bytes) the GPU writes the file's stream into it itself; pass the same array to
        wait_png."""
        assert rgb_in.dtype == np.uint8 and rgb_in.shape == (self.height, self.width, 3) and rgb_in.flags.c_contiguous
        t = C.c_uint64()
        dst, cap = (png_out.ctypes.data, png_out.size) if png_out is not None else (None, 0)
        _check(self._lib.fftup_submit_png(self._h, rgb_in.ctypes.data, 3 * self.width, dst, cap, C.byref(t)), "fftup_submit_png")
        return t.value

    def wait_png(self, ticket, buf):
        """buf: uint8 array of at least png_bound() bytes (PinnedArray for a fast copy); returns the PNG file's bytes in it"""
        assert buf.dtype == np.uint8 and buf.flags.c_contiguous
        n = C.c_size_t()
        _check(self._lib.fftup_wait_png(self._h, ticket, buf.ctypes.data, buf.size, C.byref(n)), "fftup_wait_png")
        return int(n.value)

    def wait(self, ticket):
        _check(self._lib.fftup_wait(self._h, ticket), "fftup_wait")

    def drain(self):
        _check(self._lib.fftup_drain(self._h), "fftup_drain")

    def output_checksum(self, slot=0):
        """64-bit wrapping sum of the 32-bit words of output slot `slot`, computed on the device (job accounting)."""
        v = C.c_uint64()
        _check(self._lib.fftup_output_checksum(self._h, slot, C.byref(v)), "fftup_output_checksum")
        return v.value

    def download_rgb8(self, slot=0):
        out = np.empty((self.out_height, self.out_width, 3), dtype=np.uint8)
        _check(self._lib.fftup_download_rgb8(self._h, slot, out.ctypes.data, out.strides[0]), "fftup_download_rgb8")
        return out

    # ---- frames that never leave the GPU (fftup_execute_device)
    def execute_device(self, inputs, outputs, stream=None):
        """Run the plan on caller-owned device memory: frame i reads inputs[i] (width x height) and writes outputs[i] (out_width x
        out_height).  `inputs` / `outputs`: one DeviceImage or a sequence of them per side; `stream`: a Stream, a raw hipStream_t
        value or None (the default stream).  Asynchronous: the work is ordered on `stream`, nothing waits for it here.  No ring slot
        is touched."""
        ins = [inputs] if isinstance(inputs, DeviceImage) else list(inputs)
        outs = [outputs] if isinstance(outputs, DeviceImage) else list(outputs)
        if len(ins) != len(outs):
            raise ValueError("execute_device: %d inputs, %d outputs" % (len(ins), len(outs)))
        a = (_lib.DeviceImageDesc * len(ins))(*[i.desc() for i in ins])
        b = (_lib.DeviceImageDesc * len(outs))(*[o.desc() for o in outs])
        s = stream.handle if isinstance(stream, Stream) else stream
        _check(self._lib.fftup_execute_device(self._h, a, b, len(ins), s), "fftup_execute_device")

    def execute_device_views(self, inputs, outputs, views, stream=None):
        """execute_device on a view plan with a view per frame (fftup_execute_device_views): frame i is computed with views[i] =
        (origin, span), each an (x, y) pair as Upscaler.view takes them -- views_between gives those of a move.  The tables of each
        view are built on the GPU ahead of its frame: nothing waits, the plan's own view stays what it is."""
        ins = [inputs] if isinstance(inputs, DeviceImage) else list(inputs)
        outs = [outputs] if isinstance(outputs, DeviceImage) else list(outputs)
        vws = list(views)
        if not len(ins) == len(outs) == len(vws):
            raise ValueError("execute_device_views: %d inputs, %d outputs, %d views" % (len(ins), len(outs), len(vws)))
        a = (_lib.DeviceImageDesc * len(ins))(*[i.desc() for i in ins])
        b = (_lib.DeviceImageDesc * len(outs))(*[o.desc() for o in outs])
        c = (_lib.View * len(vws))(*[_lib.View(o[0], o[1], sp[0], sp[1]) for (o, sp) in vws])
        s = stream.handle if isinstance(stream, Stream) else stream
        _check(self._lib.fftup_execute_device_views(self._h, a, b, c, len(ins), s), "fftup_execute_device_views")

    def execute_device_views_shifted(self, inputs, outputs, views, shifts_ptr, stream=None):
        """execute_device_views with frame i's origin moved by (dx, dy) of the i-th fftup_shift at `shifts_ptr`, DEVICE memory
        (fftup_execute_device_views_shifted): the GPU reads the shifts when the frame's tables are built, so what
        Aligner.shifts_device or shift_path enqueued on `stream` before is consumed without a host copy or wait."""
        ins = [inputs] if isinstance(inputs, DeviceImage) else list(inputs)
        outs = [outputs] if isinstance(outputs, DeviceImage) else list(outputs)
        vws = list(views)
        if not len(ins) == len(outs) == len(vws):
            raise ValueError("execute_device_views_shifted: %d inputs, %d outputs, %d views" % (len(ins), len(outs), len(vws)))
        a = (_lib.DeviceImageDesc * len(ins))(*[i.desc() for i in ins])
        b = (_lib.DeviceImageDesc * len(outs))(*[o.desc() for o in outs])
        c = (_lib.View * len(vws))(*[_lib.View(o[0], o[1], sp[0], sp[1]) for (o, sp) in vws])
        s = stream.handle if isinstance(stream, Stream) else stream
        _check(self._lib.fftup_execute_device_views_shifted(self._h, a, b, c, shifts_ptr, len(ins), s), "fftup_execute_device_views_shifted")

    def download_view_tables(self, lane, axis):
        """The chirp tables lane `lane` last built for axis 0 (x) or 1 (y) in execute_device_views (fftup_download_view_tables, a
        test tap): (kmax, pre, post, bhat), complex64 arrays of 2 kmax + 1, out length and L points."""
        n, m = ((self.width, self.out_width), (self.height, self.out_height))[axis] if axis in (0, 1) else (2, 2)
        need = (2 * n if self.flags & _lib.FLAG_MIRROR else 2 * (n // 2)) + m
        L = next(q for q in range(need, 4 * need + 8) if _smooth(q))
        pre = np.zeros(need - m + 1, np.complex64)
        post, bhat = np.zeros(m, np.complex64), np.zeros(L, np.complex64)
        kmax = C.c_int32()
        _check(self._lib.fftup_download_view_tables(self._h, lane, axis, pre.ctypes.data, post.ctypes.data, bhat.ctypes.data, C.byref(kmax)),
               "fftup_download_view_tables")
        return kmax.value, pre[:2 * kmax.value + 1], post, bhat


class DeviceImage:
    """One image in device memory (fftup_device_image): `ptr` an address of the plan's device, `format` FMT_RGB8 or FMT_PLANAR,
    strides in bytes (`plane_stride` is ignored for FMT_RGB8)."""

    def __init__(self, ptr, format, row_stride, plane_stride=0):
        self.ptr, self.format, self.row_stride, self.plane_stride = ptr, format, row_stride, plane_stride

    def desc(self):
        return _lib.DeviceImageDesc(self.ptr, self.format, self.row_stride, self.plane_stride)


class Stream:
    """A non-blocking HIP stream of the runtime the library uses (fftup_stream_create); `.handle` is the hipStream_t."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        h = C.c_void_p()
        _check(self._lib.fftup_stream_create(device, C.byref(h)), "fftup_stream_create")
        self.handle = h.value

    def close(self):
        if self.handle:
            h, self.handle = self.handle, None
            _check(self._lib.fftup_stream_destroy(h), "fftup_stream_destroy")

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """`nbytes` of device memory from fftup_device_alloc: what a host without HIP bindings stages frames for execute_device in.
    upload / download are blocking copies on `stream` (a Stream or None)."""

    def __init__(self, nbytes, device=0):
        self._lib = _lib.load()
        self.nbytes = int(nbytes)
        self.ptr = self._lib.fftup_device_alloc(device, self.nbytes)
        if not self.ptr:
            raise FftupError(6, "fftup_device_alloc")

    def upload(self, array, offset=0, stream=None):
        a = np.ascontiguousarray(array)
        assert 0 <= offset and offset + a.nbytes <= self.nbytes, (offset, a.nbytes, self.nbytes)
        s = stream.handle if isinstance(stream, Stream) else stream
        _check(self._lib.fftup_device_copy(self.ptr + offset, a.ctypes.data, a.nbytes, 0, s), "fftup_device_copy")

    def download(self, nbytes=None, offset=0, stream=None):
        nbytes = self.nbytes - offset if nbytes is None else int(nbytes)
        assert 0 <= offset and offset + nbytes <= self.nbytes, (offset, nbytes, self.nbytes)
        out = np.empty(nbytes, dtype=np.uint8)
        s = stream.handle if isinstance(stream, Stream) else stream
        _check(self._lib.fftup_device_copy(out.ctypes.data, self.ptr + offset, nbytes, 1, s), "fftup_device_copy")
        return out

    def close(self):
        if self.ptr:
            self._lib.fftup_device_free(self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Aligner:
    """Shift estimates between pairs of frames in device memory (fftup_align_*, include/fftup.h): band-limited phase-only correlation
    with a sub-pixel refinement, on the GPU.  `window`: (window_w, window_h) in decimated pixels or None (automatic); the zeros of
    the other arguments are the library's defaults.  `.info`: the geometry in effect and the kernel names."""

    def __init__(self, width, height, precision=0, device=0, window=None, decimate=0, band=0.0, upsample=0, max_batch=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        w = window or (0, 0)
        cfg = _lib.AlignConfig(width, height, precision, device, w[0], w[1], decimate, band, upsample, max_batch)
        _check(self._lib.fftup_align_create(C.byref(self._h), C.byref(cfg)), "fftup_align_create")
        raw = _lib.AlignInfo()
        _check(self._lib.fftup_align_get_info(self._h, C.byref(raw)), "fftup_align_get_info")
        self.info = {k: int(getattr(raw, k)) for k in ("window_w", "window_h", "decimate", "crop_x", "crop_y", "upsample", "band_kx",
                                                        "band_ky", "num_kernels", "device_bytes")}
        self.info["kernel_names"] = [bytes(n).split(b"\0")[0].decode() for n in raw.kernel_names][:raw.num_kernels]
        self.width, self.height, self.precision, self.device = width, height, precision, device

    def close(self):
        if self._h:
            self._lib.fftup_align_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def shifts_device(self, refs, curs, out_ptr, stream=None):
        """Pair i = (refs[i], curs[i]), DeviceImages of width x height (one image or a sequence per side; a single ref is repeated for
        every cur): its fftup_shift goes to out_ptr + 16 i, device memory.  Asynchronous: ordered on `stream`, nothing waits here."""
        cs = [curs] if isinstance(curs, DeviceImage) else list(curs)
        rs = [refs] * len(cs) if isinstance(refs, DeviceImage) else list(refs)
        if len(rs) != len(cs):
            raise ValueError("shifts_device: %d reference frames, %d current frames" % (len(rs), len(cs)))
        a = (_lib.DeviceImageDesc * len(rs))(*[r.desc() for r in rs])
        b = (_lib.DeviceImageDesc * len(cs))(*[c.desc() for c in cs])
        s = stream.handle if isinstance(stream, Stream) else stream
        _check(self._lib.fftup_align_shifts(self._h, a, b, len(cs), out_ptr, s), "fftup_align_shifts")

    def shifts(self, refs, curs, stream=None):
        """-> (n, 4) float32: dx, dy, peak, peak_coarse per pair, cur(x, y) ~ ref(x - dx, y - dy).  Blocking: allocates the result
        buffer, runs shifts_device and copies back on `stream`."""
        n = 1 if isinstance(curs, DeviceImage) else len(curs)
        with DeviceBuffer(max(1, n) * 16, self.device) as buf:
            self.shifts_device(refs, curs, buf.ptr, stream)
            return buf.download(stream=stream).view(np.float32).reshape(n, 4).copy()


def stabilised_views(view, shifts):
    """The `views` of Upscaler.execute_device_views that undo the estimated motion: frame i is shown at view's origin + (dx_i, dy_i),
    so it shows what the reference frame shows at the origin.  view: (origin, span); shifts: rows of Aligner.shifts (or (dx, dy) pairs)."""
    (ox, oy), span = view
    return [((float(ox) + float(s[0]), float(oy) + float(s[1])), (float(span[0]), float(span[1]))) for s in shifts]


PATH_ABSOLUTE, PATH_CONSECUTIVE, PATH_MAX_FRAMES = _lib.PATH_ABSOLUTE, _lib.PATH_CONSECUTIVE, _lib.PATH_MAX_FRAMES


def shift_path(in_ptr, out_ptr, n, mode=PATH_CONSECUTIVE, sigma=0.0, min_peak=0.0, stream=None):
    """Measured shifts -> the view offsets of a smoothed camera path (fftup_shift_path): `n` fftup_shift at `in_ptr`, device memory
    (PATH_ABSOLUTE: each against one reference; PATH_CONSECUTIVE: each against the frame before), accumulated into the path p,
    low-passed by a Gaussian of `sigma` frames into s, and p - s written as dx, dy to `out_ptr` (may be `in_ptr`) -- what
    Upscaler.execute_device_views_shifted takes.  sigma = 0: every frame locked on the reference.  Frames with peak < min_peak hold
    the path.  Asynchronous: one kernel on `stream`, nothing waits here."""
    cfg = _lib.PathConfig(mode, sigma, min_peak)
    s = stream.handle if isinstance(stream, Stream) else stream
    _check(_lib.load().fftup_shift_path(C.byref(cfg), in_ptr, out_ptr, n, s), "fftup_shift_path")


class Rotator:
    """Rotation of frames in device memory by three Fourier shears (fftup_rotate_*, include/fftup.h): every pass is the exact
    trigonometric interpolant of the frame, on the GPU.  width and height in [2, 4096], 2,3,5,7-smooth; max_batch 0: the library's
    default.  `.info`: the geometry in effect and the kernel names."""

    def __init__(self, width, height, precision=0, device=0, max_batch=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        cfg = _lib.RotateConfig(width, height, precision, device, max_batch)
        _check(self._lib.fftup_rotate_create(C.byref(self._h), C.byref(cfg)), "fftup_rotate_create")
        raw = _lib.RotateInfo()
        _check(self._lib.fftup_rotate_get_info(self._h, C.byref(raw)), "fftup_rotate_get_info")
        self.info = {k: int(getattr(raw, k)) for k in ("width", "height", "num_kernels", "max_batch", "device_bytes")}
        self.info["kernel_names"] = [bytes(n).split(b"\0")[0].decode() for n in raw.kernel_names][:raw.num_kernels]
        self.width, self.height, self.precision, self.device = width, height, precision, device

    def close(self):
        if self._h:
            self._lib.fftup_rotate_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def rotation(self, r):
        """(angle, cx, cy), or a bare angle about the frame centre ((W - 1) / 2, (H - 1) / 2) -> fftup_rotation"""
        if isinstance(r, (tuple, list)):
            angle, cx, cy = r
            return _lib.Rotation(float(angle), float(cx), float(cy))
        return _lib.Rotation(float(r), (self.width - 1) / 2.0, (self.height - 1) / 2.0)

    def rotate(self, inputs, outputs, rotations, stream=None):
        """Frame i: inputs[i] turned by rotations[i] into outputs[i] (DeviceImages of width x height; one image or a sequence per
        side; outputs[i] may be inputs[i]).  A rotation is (angle, cx, cy) in radians and pixels, or a bare angle about the frame
        centre.  A list holds one rotation per frame; a single number or one (angle, cx, cy) tuple serves every frame.  Asynchronous:
        ordered on `stream`, nothing waits here."""
        ins = [inputs] if isinstance(inputs, DeviceImage) else list(inputs)
        outs = [outputs] if isinstance(outputs, DeviceImage) else list(outputs)
        one = np.isscalar(rotations) or (isinstance(rotations, tuple) and len(rotations) == 3 and np.isscalar(rotations[0]))
        rots = [rotations] * len(ins) if one else list(rotations)
        if not len(ins) == len(outs) == len(rots):
            raise ValueError("rotate: %d inputs, %d outputs, %d rotations" % (len(ins), len(outs), len(rots)))
        a = (_lib.DeviceImageDesc * len(ins))(*[i.desc() for i in ins])
        b = (_lib.DeviceImageDesc * len(outs))(*[o.desc() for o in outs])
        c = (_lib.Rotation * len(rots))(*[self.rotation(r) for r in rots])
        s = stream.handle if isinstance(stream, Stream) else stream
        _check(self._lib.fftup_rotate_frames(self._h, a, b, c, len(ins), s), "fftup_rotate_frames")

    def frames_angles(self, inputs, outputs, rotations, angles_ptr, gain=-1.0, stream=None):
        """rotate() with frame i turned by rotations[i]'s angle + gain * the angle of the fftup_roll_angle at angles_ptr + 16 i, device
        memory -- what Roller.angles_device wrote there; the sum is formed on the GPU, the host never reads the angles.  gain = -1
        undoes a measured roll.  Asynchronous: ordered on `stream`, nothing waits here."""
        ins = [inputs] if isinstance(inputs, DeviceImage) else list(inputs)
        outs = [outputs] if isinstance(outputs, DeviceImage) else list(outputs)
        one = np.isscalar(rotations) or (isinstance(rotations, tuple) and len(rotations) == 3 and np.isscalar(rotations[0]))
        rots = [rotations] * len(ins) if one else list(rotations)
        if not len(ins) == len(outs) == len(rots):
            raise ValueError("frames_angles: %d inputs, %d outputs, %d rotations" % (len(ins), len(outs), len(rots)))
        a = (_lib.DeviceImageDesc * len(ins))(*[i.desc() for i in ins])
        b = (_lib.DeviceImageDesc * len(outs))(*[o.desc() for o in outs])
        c = (_lib.Rotation * len(rots))(*[self.rotation(r) for r in rots])
        s = stream.handle if isinstance(stream, Stream) else stream
        _check(self._lib.fftup_rotate_frames_angles(self._h, a, b, c, angles_ptr, float(gain), len(ins), s), "fftup_rotate_frames_angles")


class Roller:
    """Roll estimates between pairs of frames in device memory (fftup_roll_*, include/fftup.h): the rotation about the optical axis
    from the spectra's magnitudes on a polar grid, phase-only correlation along the angle with a sub-sample refinement, on the GPU.
    `window`: (window_w, window_h) in decimated pixels or None (automatic); the zeros of the other arguments are the library's
    defaults.  `.info`: the geometry in effect and the kernel names."""

    def __init__(self, width, height, precision=0, device=0, window=None, decimate=0, band=0.0, angles=0, upsample=0, max_batch=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        w = window or (0, 0)
        cfg = _lib.RollConfig(width, height, precision, device, w[0], w[1], decimate, band, angles, upsample, max_batch)
        _check(self._lib.fftup_roll_create(C.byref(self._h), C.byref(cfg)), "fftup_roll_create")
        raw = _lib.RollInfo()
        _check(self._lib.fftup_roll_get_info(self._h, C.byref(raw)), "fftup_roll_get_info")
        self.info = {k: int(getattr(raw, k)) for k, _ in _lib.RollInfo._fields_ if k != "kernel_names"}
        self.info["kernel_names"] = [bytes(n).split(b"\0")[0].decode() for n in raw.kernel_names][:raw.num_kernels]
        self.width, self.height, self.precision, self.device = width, height, precision, device

    def close(self):
        if self._h:
            self._lib.fftup_roll_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def angles_device(self, refs, curs, out_ptr, stream=None):
        """Pair i = (refs[i], curs[i]), DeviceImages of width x height (one image or a sequence per side; a single ref is repeated for
        every cur): its fftup_roll_angle goes to out_ptr + 16 i, device memory.  Asynchronous: ordered on `stream`, nothing waits here."""
        cs = [curs] if isinstance(curs, DeviceImage) else list(curs)
        rs = [refs] * len(cs) if isinstance(refs, DeviceImage) else list(refs)
        if len(rs) != len(cs):
            raise ValueError("angles_device: %d reference frames, %d current frames" % (len(rs), len(cs)))
        a = (_lib.DeviceImageDesc * len(rs))(*[r.desc() for r in rs])
        b = (_lib.DeviceImageDesc * len(cs))(*[c.desc() for c in cs])
        s = stream.handle if isinstance(stream, Stream) else stream
        _check(self._lib.fftup_roll_angles(self._h, a, b, len(cs), out_ptr, s), "fftup_roll_angles")

    def angles(self, refs, curs, stream=None):
        """-> (n, 4) float32: angle, peak, peak_coarse, 0 per pair, cur ~ ref turned by +angle radians.  Blocking: allocates the
        result buffer, runs angles_device and copies back on `stream`."""
        n = 1 if isinstance(curs, DeviceImage) else len(curs)
        with DeviceBuffer(max(1, n) * 16, self.device) as buf:
            self.angles_device(refs, curs, buf.ptr, stream)
            return buf.download(stream=stream).view(np.float32).reshape(n, 4).copy()


class PinnedArray:
    """uint8 numpy view of page-locked host memory from fftup_host_alloc (needed for truly asynchronous copies
    in Upscaler.submit_rgb8); free with .close() after the frames using it have been waited for."""

    def __init__(self, shape):
        self._lib = _lib.load()
        n = int(np.prod(shape))
        self._p = self._lib.fftup_host_alloc(n)
        if not self._p:
            raise FftupError(5, "fftup_host_alloc")
        self.array = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_uint8)), shape=(n,)).reshape(shape)

    def close(self):
        if self._p:
            self.array = None
            self._lib.fftup_host_free(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def view_of_rect(x0, y0, w, h, out_width, out_height):
    """(origin, span) of Upscaler.view for the rectangle [x0, x0 + w) x [y0, y0 + h) in pixel-EDGE coordinates (pixel n covers
    [n, n + 1)), pixel centres aligned: per axis origin = x0 + w / (2 M) - 1/2, span = w."""
    return ((x0 + w / (2.0 * out_width) - 0.5, y0 + h / (2.0 * out_height) - 0.5), (float(w), float(h)))


def views_between(v0, v1, n):
    """The n views of a move from v0 to v1 (each (origin, span), (x, y) pairs), for Upscaler.execute_device_views.  Frame k, t = k / (n - 1):
    per axis the origin is linear in t, (1 - t) o0 + t o1, the span geometric, span0 (span1 / span0) ** t -- a zoom at a constant
    rate.  The first view is v0 and the last v1, exactly; n = 1 gives [v0]."""
    def as_view(v):
        return ((float(v[0][0]), float(v[0][1])), (float(v[1][0]), float(v[1][1])))
    v0, v1 = as_view(v0), as_view(v1)
    out = []
    for k in range(n):
        if k == 0 or k == n - 1:
            out.append(v0 if k == 0 else v1)
            continue
        t = k / (n - 1)
        out.append((tuple((1.0 - t) * a + t * b for a, b in zip(v0[0], v1[0])), tuple(a * (b / a) ** t for a, b in zip(v0[1], v1[1]))))
    return out


def _smooth(n):
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def upscale_image(rgb, upscale=2.0, precision=0, sharpen=0.2, num_iter=1, device=0, flags=0):
    """Single-image path of launchResample(): returns (rgb_out uint8 [uH][uW][3], ms_per_iter)."""
    rgb = np.asarray(rgb)
    with Upscaler(rgb.shape[1], rgb.shape[0], upscale, precision, sharpen, device, flags) as up:
        up.upload_rgb8(rgb)
        ms = up.execute(num_iter)
        return up.download_rgb8(), ms
