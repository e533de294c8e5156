// fftup_align.hip -- shift estimates: the aligner object of include/fftup.h (fftup_align_create / _destroy / _get_info / _shifts) and the
// launches of its kernels (kernels_align.hpp).  The geometry comes from align_geometry (plan_rules.cpp), before any device access;
// tables and the buffers of max_batch pairs are made at creation; fftup_align_shifts validates, then only launches.
// And fftup_shift_path, which needs no aligner: measured shifts -> the view offsets of a smoothed camera path (shift_path.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "kernels_align.hpp"
#include "plan.hpp"
#include "shift_path.hpp"

using namespace fftup;

struct fftup_align {
    AlignGeometry g;
    int device = 0;
    size_t esz = 4;                   // bytes of a FFTUP_FMT_PLANAR element
    AlignParams p{};
    int thrX = 64, thrY = 64;         // threads of the row kernels / the column kernel
    std::vector<void*> allocs;
    uint64_t device_bytes = 0;
};

namespace {

const char* const KERNEL_NAMES[] = {"align_rows", "align_cols", "align_peak_rows", "align_fine_x", "align_fine_y"};
constexpr int NUM_KERNELS = 5;
constexpr int FINE_THREADS = 128, FINAL_THREADS = 256;

struct AlignDestroyer { void operator()(fftup_align* a) const { fftup_align_destroy(a); } };

int align_alloc(fftup_align* a, void** ptr, size_t bytes)
{
    const hipError_t e = hipMalloc(ptr, bytes);
    if (e != hipSuccess) {
        *ptr = nullptr;
        (void)hipGetLastError();
        return fail(FFTUP_E_OUT_OF_MEMORY, std::string("fftup_align_create: hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    }
    a->allocs.push_back(*ptr);
    a->device_bytes += bytes;
    return FFTUP_OK;
}

template <class T> int align_upload(fftup_align* a, const T** dptr, const std::vector<T>& h)
{
    void* d = nullptr;
    if (int rc = align_alloc(a, &d, sizeof(T) * h.size())) return rc;
    HIP_TRY(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    *dptr = (const T*)d;
    return FFTUP_OK;
}

// the m-th roots exp(+2 pi i k / m) in double, rounded once to fp32
std::vector<float2> roots(uint32_t m)
{
    std::vector<float2> h(m);
    for (uint32_t k = 0; k < m; k++) {
        const double t = 2.0 * M_PI * (double)k / (double)m;
        h[k] = make_float2((float)std::cos(t), (float)std::sin(t));
    }
    return h;
}

std::vector<float> window(uint32_t n)
{
    std::vector<float> w(n);
    for (uint32_t k = 0; k < n; k++) w[k] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * ((double)k + 0.5) / (double)n));
    return w;
}

int fft_threads(uint32_t points) { return (int)std::min(256u, std::max(64u, points / 4)); }

size_t rows_lds(const fftup_align* a) { return 2 * sizeof(float2) * (size_t)lpad_size((int)a->g.nx); }
size_t cols_lds(const fftup_align* a) { return sizeof(float2) * (2 * (size_t)lpad_size(2 * (int)a->g.ny) + (size_t)a->thrY); }

AlignImage image_of(const fftup_align* a, const fftup_device_image& im)
{
    AlignImage r;
    r.data = (const uint8_t*)im.data;
    r.row = (long)im.row_stride_bytes;
    r.plane = (long)im.plane_stride_bytes;
    if (im.format == FFTUP_FMT_RGB8) r.kind = 0;
    else {
        const bool aligned = (uintptr_t)im.data % a->esz == 0;
        r.kind = a->esz == 4 ? (aligned ? 1 : 3) : (aligned ? 2 : 4);
    }
    return r;
}

}  // namespace

extern "C" {

int fftup_align_create(fftup_align** out, const fftup_align_config* cfg)
{
    if (!out || !cfg) return fail(FFTUP_E_INVALID_ARG, "fftup_align_create: null argument");
    *out = nullptr;
    AlignGeometry G;
    if (int rc = align_geometry(*cfg, G)) return rc;          // (before any device access)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); ndev = 0; }
    if (ndev <= 0) return fail(FFTUP_E_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(FFTUP_E_NO_DEVICE, "device id out of range");

    std::unique_ptr<fftup_align, AlignDestroyer> owner(new fftup_align());
    fftup_align* a = owner.get();
    a->g = G;
    a->device = cfg->device;
    a->esz = G.precision == 2 ? 2 : 4;
    a->thrX = fft_threads(G.nx);
    a->thrY = fft_threads(G.ny);
    HIP_TRY(hipSetDevice(a->device));
    AlignParams& p = a->p;
    p.nx = (int)G.nx; p.ny = (int)G.ny; p.d = (int)G.d; p.crop_x = (int)G.crop_x; p.crop_y = (int)G.crop_y; p.kappa = (int)G.kappa;
    p.bkx = (int)G.band_kx; p.bky = (int)G.band_ky; p.Kx = (int)G.Kx; p.Ky = (int)G.Ky;
    p.planX = make_stage_plan(G.nx);
    p.planY = make_stage_plan(G.ny);
    int rc;
    if ((rc = align_upload(a, &p.twX, roots(G.nx)))) return rc;
    if ((rc = align_upload(a, &p.twY, roots(G.ny)))) return rc;
    if ((rc = align_upload(a, &p.winX, window(G.nx)))) return rc;
    if ((rc = align_upload(a, &p.winY, window(G.ny)))) return rc;
    if ((rc = align_upload(a, &p.phX, roots(G.kappa * G.nx)))) return rc;
    if ((rc = align_upload(a, &p.phY, roots(G.kappa * G.ny)))) return rc;
    const size_t B = G.max_batch, nf = 2 * (size_t)G.kappa + 1;
    if ((rc = align_alloc(a, (void**)&p.Z, sizeof(float2) * B * G.nx * G.ny))) return rc;
    if ((rc = align_alloc(a, (void**)&p.dc, sizeof(float2) * B * G.ny))) return rc;
    if ((rc = align_alloc(a, (void**)&p.Rb, sizeof(float2) * B * G.Kx * G.Ky))) return rc;
    if ((rc = align_alloc(a, (void**)&p.Gx, sizeof(float2) * B * G.Ky * nf))) return rc;
    if ((rc = align_alloc(a, (void**)&p.part, sizeof(float2) * B * G.ny))) return rc;
    *out = owner.release();
    return FFTUP_OK;
}

void fftup_align_destroy(fftup_align* a)
{
    if (!a) return;
    if (!a->allocs.empty()) {
        (void)hipSetDevice(a->device);
        (void)hipDeviceSynchronize();
        for (void* q : a->allocs) (void)hipFree(q);
    }
    delete a;
}

int fftup_align_get_info(const fftup_align* a, fftup_align_info* info)
{
    if (!a || !info) return fail(FFTUP_E_INVALID_ARG, "fftup_align_get_info: null argument");
    memset(info, 0, sizeof(*info));
    info->window_w = a->g.nx; info->window_h = a->g.ny; info->decimate = a->g.d;
    info->crop_x = a->g.crop_x; info->crop_y = a->g.crop_y; info->upsample = a->g.kappa;
    info->band_kx = a->g.band_kx; info->band_ky = a->g.band_ky;
    info->num_kernels = NUM_KERNELS;
    info->device_bytes = a->device_bytes;
    for (int k = 0; k < NUM_KERNELS; k++) snprintf(info->kernel_names[k], sizeof(info->kernel_names[k]), "%s", KERNEL_NAMES[k]);
    return FFTUP_OK;
}

int fftup_align_shifts(fftup_align* a, const fftup_device_image* ref, const fftup_device_image* cur, uint32_t n_pairs,
                       fftup_shift* shifts_device, void* stream)
{
    if (!a) return fail(FFTUP_E_INVALID_ARG, "fftup_align_shifts: null aligner");
    if (!ref || !cur) return fail(FFTUP_E_INVALID_ARG, "fftup_align_shifts: null image array");
    if (!shifts_device) return fail(FFTUP_E_INVALID_ARG, "fftup_align_shifts: shifts_device is null");
    if (n_pairs == 0) return fail(FFTUP_E_INVALID_ARG, "fftup_align_shifts: n_pairs must be > 0");
    HIP_TRY(hipSetDevice(a->device));
    // ---- everything that can be refused is refused here, before the first launch
    for (uint32_t i = 0; i < n_pairs; i++) {
        int rc = check_device_image(a->esz, false, a->device, ref[i], "ref", i, a->g.W, a->g.H, false);
        if (!rc) rc = check_device_image(a->esz, false, a->device, cur[i], "cur", i, a->g.W, a->g.H, false);
        if (rc) return rc;
    }
    if ((uintptr_t)shifts_device % sizeof(float)) return fail(FFTUP_E_INVALID_ARG, "fftup_align_shifts: shifts_device is not a multiple of 4 bytes");
    {
        hipPointerAttribute_t at{};
        const hipError_t e = hipPointerGetAttributes(&at, shifts_device);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(FFTUP_E_INVALID_ARG, std::string("fftup_align_shifts: shifts_device is not device memory (hipPointerGetAttributes: ") + hipGetErrorString(e) + ")");
        }
        if (at.type != hipMemoryTypeDevice || at.device != a->device)
            return fail(FFTUP_E_INVALID_ARG, "fftup_align_shifts: shifts_device is not device memory of the aligner's device");
    }
    hipStream_t st = (hipStream_t)stream;
    const AlignGeometry& g = a->g;
    const AlignParams& p = a->p;
    const uint32_t col_pairs = std::min(g.band_kx, g.nx / 2) + 1;
    for (uint32_t base = 0; base < n_pairs; base += g.max_batch) {       // a chunk reuses the buffers of the one before: stream order
        const uint32_t n = std::min(g.max_batch, n_pairs - base);
        for (uint32_t s = 0; s < n; s += ALIGN_PAIRS_PER_LAUNCH) {
            const uint32_t m = std::min<uint32_t>(ALIGN_PAIRS_PER_LAUNCH, n - s);
            AlignPairs q{};
            for (uint32_t k = 0; k < m; k++) {
                q.ref[k] = image_of(a, ref[base + s + k]);
                q.cur[k] = image_of(a, cur[base + s + k]);
            }
            hipLaunchKernelGGL(k_align_rows, dim3(g.ny, 1, m), dim3(a->thrX), rows_lds(a), st, p, q, (int)s);
        }
        hipLaunchKernelGGL(k_align_cols, dim3(col_pairs, 1, n), dim3(a->thrY), cols_lds(a), st, p);
        hipLaunchKernelGGL(k_align_peak_rows, dim3(g.ny, 1, n), dim3(a->thrX), rows_lds(a), st, p);
        hipLaunchKernelGGL(k_align_fine_x, dim3(g.Ky, 1, n), dim3(FINE_THREADS), 0, st, p);
        hipLaunchKernelGGL(k_align_fine_y, dim3(1, 1, n), dim3(FINAL_THREADS), 0, st, p, (float*)(shifts_device + base));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(FFTUP_E_HIP, std::string("fftup_align_shifts: kernel launch: ") + hipGetErrorString(e));
    }
    return FFTUP_OK;
}

// measured shifts -> the view offsets of a smoothed camera path (shift_path.hpp has the definition): the rules on the numbers first,
// before any device access; then the pointers, whose attributes name the device; then one launch
int fftup_shift_path(const fftup_path_config* cfg, const fftup_shift* in_device, fftup_shift* out_device, uint32_t n_frames, void* stream)
{
    if (!cfg) return fail(FFTUP_E_INVALID_ARG, "fftup_shift_path: cfg is null");
    if (!in_device) return fail(FFTUP_E_INVALID_ARG, "fftup_shift_path: in_device is null");
    if (!out_device) return fail(FFTUP_E_INVALID_ARG, "fftup_shift_path: out_device is null");
    if (n_frames == 0) return fail(FFTUP_E_INVALID_ARG, "fftup_shift_path: n_frames must be > 0");
    if (n_frames > (uint32_t)FFTUP_PATH_MAX_FRAMES)
        return fail(FFTUP_E_INVALID_ARG, "fftup_shift_path: n_frames " + std::to_string(n_frames) + " is above FFTUP_PATH_MAX_FRAMES (" + std::to_string((int)FFTUP_PATH_MAX_FRAMES) + ")");
    if (cfg->mode > 1) return fail(FFTUP_E_INVALID_ARG, "fftup_shift_path: mode must be FFTUP_PATH_ABSOLUTE (0) or FFTUP_PATH_CONSECUTIVE (1)");
    if (!(std::isfinite(cfg->sigma) && cfg->sigma >= 0.0f && cfg->sigma <= fftup_shiftpath::MAX_SIGMA))
        return fail(FFTUP_E_INVALID_ARG, "fftup_shift_path: sigma must be a finite number in [0, 256]");
    if (!std::isfinite(cfg->min_peak)) return fail(FFTUP_E_INVALID_ARG, "fftup_shift_path: min_peak must be a finite number");
    int device = -1;
    const struct { const void* p; const char* name; } ptrs[2] = {{in_device, "in_device"}, {out_device, "out_device"}};
    for (const auto& q : ptrs) {
        const std::string at = std::string("fftup_shift_path: ") + q.name;
        if ((uintptr_t)q.p % sizeof(float)) return fail(FFTUP_E_INVALID_ARG, at + " is not a multiple of 4 bytes");
        hipPointerAttribute_t a{};
        const hipError_t e = hipPointerGetAttributes(&a, q.p);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(FFTUP_E_INVALID_ARG, at + " is not device memory (hipPointerGetAttributes: " + hipGetErrorString(e) + ")");
        }
        if (a.type != hipMemoryTypeDevice) return fail(FFTUP_E_INVALID_ARG, at + " is not device memory");
        if (device >= 0 && a.device != device) return fail(FFTUP_E_INVALID_ARG, "fftup_shift_path: in_device and out_device are not memory of one and the same device");
        device = a.device;
    }
    HIP_TRY(hipSetDevice(device));
    return launch_shift_path(in_device, out_device, n_frames, cfg->mode, cfg->sigma, cfg->min_peak, (hipStream_t)stream);
}

}  // extern "C"
