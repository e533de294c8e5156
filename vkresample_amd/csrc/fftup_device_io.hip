// fftup_device_io.hip -- frames that never leave the GPU: fftup_execute_device runs a plan on caller-owned device memory (the
// frame's first kernel reads the caller's image, its last kernel writes the caller's image, in place wherever the layout allows),
// and the helper family that lets a host without HIP bindings stage device data through the runtime this library uses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "plan.hpp"

// every rule of include/fftup.h for one descriptor; `w` x `h`: the image it names (plan.hpp: fftup_align_shifts checks with it too)
int check_device_image(size_t esz, bool u8out, int device, const fftup_device_image& im, const char* side, uint32_t i, uint32_t w, uint32_t h, bool is_out)
{
    const std::string at = std::string(side) + "[" + std::to_string(i) + "]";
    if (!im.data) return fail(FFTUP_E_INVALID_ARG, at + ".data is null");
    if (im.format != FFTUP_FMT_RGB8 && im.format != FFTUP_FMT_PLANAR) return fail(FFTUP_E_INVALID_ARG, at + ".format " + std::to_string(im.format) + " is not a FFTUP_FMT_* format");
    if (im.format == FFTUP_FMT_RGB8) {
        if (im.row_stride_bytes < (size_t)3 * w)
            return fail(FFTUP_E_INVALID_ARG, at + ".row_stride_bytes " + std::to_string(im.row_stride_bytes) + " is below one row of " + std::to_string((size_t)3 * w) + " bytes");
    } else {
        if (is_out && u8out)
            return fail(FFTUP_E_INVALID_ARG, at + ": the plan stores 8-bit RGB only (FFTUP_FLAG_FUSE_U8_STORE), it has no planes: use FFTUP_FMT_RGB8");
        if (im.row_stride_bytes < (size_t)w * esz)
            return fail(FFTUP_E_INVALID_ARG, at + ".row_stride_bytes " + std::to_string(im.row_stride_bytes) + " is below one row of " + std::to_string((size_t)w * esz) + " bytes");
        if (im.row_stride_bytes % esz)
            return fail(FFTUP_E_INVALID_ARG, at + ".row_stride_bytes " + std::to_string(im.row_stride_bytes) + " is not a multiple of the element size " + std::to_string(esz));
        if (im.plane_stride_bytes < (size_t)h * im.row_stride_bytes)
            return fail(FFTUP_E_INVALID_ARG, at + ".plane_stride_bytes " + std::to_string(im.plane_stride_bytes) + " is below height * row_stride_bytes");
        if (im.plane_stride_bytes % esz)
            return fail(FFTUP_E_INVALID_ARG, at + ".plane_stride_bytes " + std::to_string(im.plane_stride_bytes) + " is not a multiple of the element size " + std::to_string(esz));
    }
    hipPointerAttribute_t a{};
    const hipError_t e = hipPointerGetAttributes(&a, im.data);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FFTUP_E_INVALID_ARG, at + ".data is not device memory (hipPointerGetAttributes: " + hipGetErrorString(e) + ")");
    }
    if (a.type != hipMemoryTypeDevice) return fail(FFTUP_E_INVALID_ARG, at + ".data is not device memory");
    if (a.device != device) return fail(FFTUP_E_INVALID_ARG, at + ".data is device memory of device " + std::to_string(a.device) + ", the plan runs on device " + std::to_string(device));
    return FFTUP_OK;
}

namespace {

// one side of one frame, decided from the descriptor alone (nothing here touches the memory)
struct Route {
    bool in_place = false;   // the frame kernel reads / writes `data` itself
    int gran = 1;            // otherwise: the copy kernel's granularity
};

int check_image(const fftup_plan* P, const fftup_device_image& im, const char* side, uint32_t i, uint32_t w, uint32_t h, bool is_out)
{
    return check_device_image(P->esz, P->u8out, P->device, im, side, i, w, h, is_out);
}

// Input planes run in place when `data` is a multiple of the element size: every first kernel of a frame (load_px, load_px_t: the
// size-generic, ahead-of-time, plan-time, four-step, non-R2C, DCT, downscale, Bluestein and odd-size row kernels) loads single
// elements at c * plane_stride + y * row_stride + x, computed in 64 bits.  8-bit rows are read byte by byte: any address.
Route route_in(const fftup_plan* P, const fftup_device_image& im)
{
    Route r;
    if (im.format == FFTUP_FMT_RGB8) { r.in_place = fuse_u8(P); return r; }
    r.in_place = (uintptr_t)im.data % P->esz == 0;
    return r;
}

// Output runs in place when it is dense and, for planes, `data` is 16-byte aligned: k_sharpen_t, k_sharpen_f64 and the fused
// C2R+sharpen kernels (ahead-of-time and plan-time) store 8 or 16 bytes at once at multiples of four (two) pixels from `data`;
// k_sharpen and k_sharpen_c store single elements, the fused 8-bit store single bytes.  None of them writes behind the image's
// 3 uW uH elements (the + 8 bytes of a slot are there for k_checksum, k_pack_u8 and k_png_filter, which READ whole words).
Route route_out(const fftup_plan* P, const fftup_device_image& im)
{
    Route r;
    if (im.format == FFTUP_FMT_RGB8) {
        r.in_place = P->u8out && im.row_stride_bytes == (size_t)3 * P->uW;
        return r;
    }
    r.in_place = im.row_stride_bytes == (size_t)P->uW * P->esz && im.plane_stride_bytes == (size_t)P->uW * P->uH * P->esz && (uintptr_t)im.data % 16 == 0;
    r.gran = (uintptr_t)im.data % P->esz == 0 ? (int)P->esz : 1;
    return r;
}

int ensure_events(fftup_plan* P)
{
    if (P->dio.start) return FFTUP_OK;
    HIP_TRY(hipEventCreateWithFlags(&P->dio.start, hipEventDisableTiming));
    P->dio.stage_in.assign(P->nlanes, nullptr);
    P->dio.scratch_out.assign(P->nlanes, nullptr);
    return FFTUP_OK;
}

// fftup_execute_device, and with `views` fftup_execute_device_views: frame i computed with views[i] instead of the plan's view;
// with `shifts` as well fftup_execute_device_views_shifted (`who` names the entry point): frame i's table kernel moves the origin of
// views[i] by shifts[i] in device memory -- checked here as fftup_align_shifts checks its own shifts_device, never read here
int execute_device(fftup_plan* P, const fftup_device_image* in, const fftup_device_image* out, const fftup_view* views, const fftup_shift* shifts,
                   const char* who, uint32_t n_frames, void* stream)
{
    if (!P) return fail(FFTUP_E_INVALID_ARG, "null plan");
    if (!in || !out) return fail(FFTUP_E_INVALID_ARG, "null image array");
    if (n_frames == 0) return fail(FFTUP_E_INVALID_ARG, "n_frames must be > 0");
    HIP_TRY(hipSetDevice(P->device));
    // ---- everything that can be refused is refused here, before the first launch
    for (uint32_t i = 0; i < n_frames; i++) {
        int rc = check_image(P, in[i], "in", i, P->W, P->H, false);
        if (!rc) rc = check_image(P, out[i], "out", i, P->uW, P->uH, true);
        if (!rc && views) rc = check_view((std::string(who) + ": views[" + std::to_string(i) + "]").c_str(), &views[i], P->uW, P->uH);
        if (rc) return rc;
    }
    if (shifts) {
        if ((uintptr_t)shifts % sizeof(float)) return fail(FFTUP_E_INVALID_ARG, std::string(who) + ": shifts_device is not a multiple of 4 bytes");
        hipPointerAttribute_t at{};
        const hipError_t e = hipPointerGetAttributes(&at, shifts);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(FFTUP_E_INVALID_ARG, std::string(who) + ": shifts_device is not device memory (hipPointerGetAttributes: " + hipGetErrorString(e) + ")");
        }
        if (at.type != hipMemoryTypeDevice || at.device != P->device)
            return fail(FFTUP_E_INVALID_ARG, std::string(who) + ": shifts_device is not device memory of the plan's device");
    }
    int rc = ensure_events(P);
    if (rc) return rc;
    // consecutive frames alternate on the plan's lanes, as in fftup_execute_ring
    const int nl = (int)std::min<uint32_t>((uint32_t)P->nlanes, n_frames);
    if (views && (rc = view_frames_prepare(P, nl))) return rc;          // (the lanes' table sets, on first use)
    const size_t esz = P->esz, out_bytes = (size_t)3 * P->uW * P->uH * (P->u8out ? 1 : esz);
    for (uint32_t i = 0; i < n_frames; i++) {                 // the staging of the layouts that cannot run in place, on first use
        const int l = (int)(i % (uint32_t)nl);
        if (!route_in(P, in[i]).in_place && !P->dio.stage_in[l] && (rc = dev_alloc(P, &P->dio.stage_in[l], 3 * P->in_plane_stride * esz))) return rc;
        if (!route_out(P, out[i]).in_place && !P->dio.scratch_out[l] && (rc = dev_alloc(P, &P->dio.scratch_out[l], out_bytes + 8))) return rc;
    }
    hipStream_t cs = (hipStream_t)stream;
    if ((rc = lanes_fork(P, P->dio.start, cs, 0, nl))) return rc;
    for (uint32_t i = 0; i < n_frames && !rc; i++) {
        const int l = (int)(i % (uint32_t)nl);
        hipStream_t st = P->lanes[l].stream;
        const fftup_device_image &src = in[i], &dst = out[i];
        const Route ri = route_in(P, src), ro = route_out(P, dst);
        DeviceInput io;
        if (src.format == FFTUP_FMT_RGB8 && ri.in_place) {    // FFTUP_FLAG_FUSE_U8_LOAD: the row kernel reads the caller's bytes
            io.in = src.data; io.kind = 2; io.in_row = (long)src.row_stride_bytes;
        } else if (ri.in_place) {
            io.in = src.data; io.kind = 1; io.in_row = (long)(src.row_stride_bytes / esz); io.in_plane = (long)(src.plane_stride_bytes / esz);
        } else {
            void* stage = P->dio.stage_in[l];
            if (src.format == FFTUP_FMT_RGB8) launch_unpack_from(P, (const uint8_t*)src.data, src.row_stride_bytes, stage, st);
            else launch_copy_rows(src.data, src.row_stride_bytes, src.plane_stride_bytes, stage, P->W * esz, P->in_plane_stride * esz,
                                  P->W * esz, P->H, 3, 1, st);             // (the source is not element aligned: bytes)
            io.in = stage; io.kind = 1; io.in_row = (long)P->W; io.in_plane = (long)P->in_plane_stride;
        }
        const FrameRun r{l, 0, ro.in_place ? dst.data : P->dio.scratch_out[l], &io, Pass::all, views ? &views[i] : nullptr, shifts ? &shifts[i] : nullptr};
        if ((rc = launch_frame(P, r))) break;
        if (!ro.in_place) {
            if (dst.format == FFTUP_FMT_PLANAR)
                launch_copy_rows(r.out, P->uW * esz, (size_t)P->uW * P->uH * esz, dst.data, dst.row_stride_bytes, dst.plane_stride_bytes,
                                 P->uW * esz, P->uH, 3, ro.gran, st);
            else if (P->u8out)
                launch_copy_rows(r.out, (size_t)3 * P->uW, 0, dst.data, dst.row_stride_bytes, 0, (size_t)3 * P->uW, P->uH, 1, 1, st);
            else launch_pack_to(P, r.out, (uint8_t*)dst.data, dst.row_stride_bytes, st);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fail(FFTUP_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    }
    // `stream` goes on behind every lane used; so does the plan's own stream, on which the taps and every other entry point run
    // (lane 0 runs on the plan's own stream)
    rc = lanes_join(P, 0, nl, {cs, P->stream}, rc);
    if (!rc) P->dev_executed = true;
    return rc;
}

}  // namespace

extern "C" {

int fftup_execute_device(fftup_plan* P, const fftup_device_image* in, const fftup_device_image* out, uint32_t n_frames, void* stream)
{
    return execute_device(P, in, out, nullptr, nullptr, "fftup_execute_device", n_frames, stream);
}

int fftup_execute_device_views(fftup_plan* P, const fftup_device_image* in, const fftup_device_image* out, const fftup_view* views,
                               uint32_t n_frames, void* stream)
{
    if (!P) return fail(FFTUP_E_INVALID_ARG, "null plan");
    if (!views) return fail(FFTUP_E_INVALID_ARG, "fftup_execute_device_views: views is null");
    if (!P->view) return fail(FFTUP_E_INVALID_ARG, "fftup_execute_device_views: not a view plan (fftup_plan_create_view makes one)");
    return execute_device(P, in, out, views, nullptr, "fftup_execute_device_views", n_frames, stream);
}

int fftup_execute_device_views_shifted(fftup_plan* P, const fftup_device_image* in, const fftup_device_image* out, const fftup_view* views,
                                       const fftup_shift* shifts_device, uint32_t n_frames, void* stream)
{
    if (!P) return fail(FFTUP_E_INVALID_ARG, "null plan");
    if (!views) return fail(FFTUP_E_INVALID_ARG, "fftup_execute_device_views_shifted: views is null");
    if (!shifts_device) return fail(FFTUP_E_INVALID_ARG, "fftup_execute_device_views_shifted: shifts_device is null");
    if (!P->view) return fail(FFTUP_E_INVALID_ARG, "fftup_execute_device_views_shifted: not a view plan (fftup_plan_create_view makes one)");
    return execute_device(P, in, out, views, shifts_device, "fftup_execute_device_views_shifted", n_frames, stream);
}

// the parity tests' tap: the tables lane `lane` last built for axis 0 (x) or 1 (y)
int fftup_download_view_tables(fftup_plan* P, uint32_t lane, uint32_t axis, float* pre, float* post, float* bhat, int32_t* kmax)
{
    if (!P) return fail(FFTUP_E_INVALID_ARG, "null plan");
    if (!P->view) return fail(FFTUP_E_INVALID_ARG, "fftup_download_view_tables: not a view plan (fftup_plan_create_view makes one)");
    if (axis > 1) return fail(FFTUP_E_INVALID_ARG, "fftup_download_view_tables: axis must be 0 (x) or 1 (y)");
    if (lane >= (uint32_t)P->nlanes) return fail(FFTUP_E_INVALID_ARG, "fftup_download_view_tables: lane out of range");
    if (lane >= P->vtabs.size() || !P->vtabs[lane].built) return fail(FFTUP_E_INVALID_ARG, "fftup_download_view_tables: this lane has built no tables yet (fftup_execute_device_views does)");
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(hipStreamSynchronize(P->lanes[lane].stream));
    const fftup_plan::ViewTabs& t = P->vtabs[lane];
    const size_t M = axis ? P->uH : P->uW, L = axis ? P->vy.L : P->vx.L, K = 2 * (size_t)t.kmax[axis] + 1;
    if (pre) HIP_TRY(hipMemcpy(pre, t.pre[axis], sizeof(float2) * K, hipMemcpyDeviceToHost));
    if (post) HIP_TRY(hipMemcpy(post, t.post[axis], sizeof(float2) * M, hipMemcpyDeviceToHost));
    if (bhat) HIP_TRY(hipMemcpy(bhat, t.bhat[axis], sizeof(float2) * L, hipMemcpyDeviceToHost));
    if (kmax) *kmax = t.kmax[axis];
    return FFTUP_OK;
}

void* fftup_device_alloc(int device, size_t bytes)
{
    void* p = nullptr;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fail(e == hipErrorOutOfMemory ? FFTUP_E_OUT_OF_MEMORY : FFTUP_E_HIP, std::string("fftup_device_alloc: ") + hipGetErrorString(e));
        return nullptr;
    }
    return p;
}

void fftup_device_free(void* ptr)
{
    if (ptr) (void)hipFree(ptr);
}

int fftup_device_copy(void* dst, const void* src, size_t bytes, int kind, void* stream)
{
    if (!dst || !src) return fail(FFTUP_E_INVALID_ARG, "null pointer");
    if (kind < 0 || kind > 2) return fail(FFTUP_E_INVALID_ARG, "kind must be 0 (host to device), 1 (device to host) or 2 (device to device)");
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, k, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return FFTUP_OK;
}

int fftup_stream_create(int device, void** stream)
{
    if (!stream) return fail(FFTUP_E_INVALID_ARG, "null pointer");
    *stream = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        (void)hipGetLastError();
        return fail(FFTUP_E_NO_DEVICE, "bad device id");
    }
    HIP_TRY(hipSetDevice(device));
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void*)s;
    return FFTUP_OK;
}

int fftup_stream_destroy(void* stream)
{
    if (!stream) return fail(FFTUP_E_INVALID_ARG, "null stream");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return FFTUP_OK;
}

}  // extern "C"
