// fftup_roll.hip -- roll estimates: the estimator object of include/fftup.h (fftup_roll_create / _destroy / _get_info / _angles) and
// the launches of its kernels (kernels_roll.hpp).  The geometry comes from roll_geometry (plan_rules.cpp), before any device access;
// tables and the buffers of max_batch pairs are made at creation; fftup_roll_angles validates, then only launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "kernels_roll.hpp"
#include "plan.hpp"

using namespace fftup;

struct fftup_roll {
    RollGeometry g;
    int device = 0;
    size_t esz = 4;                   // bytes of a FFTUP_FMT_PLANAR element
    RollParams p{};
    int thrX = 64, thrY = 64, thrT = 64;   // threads of the row, column and polar kernels
    std::vector<void*> allocs;
    uint64_t device_bytes = 0;
};

namespace {

const char* const KERNEL_NAMES[] = {"roll_rows", "roll_cols", "roll_polar", "roll_peak"};
constexpr int NUM_KERNELS = 4;
constexpr int PEAK_THREADS = 256;

struct RollDestroyer { void operator()(fftup_roll* r) const { fftup_roll_destroy(r); } };

int roll_alloc(fftup_roll* r, void** ptr, size_t bytes)
{
    const hipError_t e = hipMalloc(ptr, bytes);
    if (e != hipSuccess) {
        *ptr = nullptr;
        (void)hipGetLastError();
        return fail(FFTUP_E_OUT_OF_MEMORY, std::string("fftup_roll_create: hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    }
    r->allocs.push_back(*ptr);
    r->device_bytes += bytes;
    return FFTUP_OK;
}

template <class T> int roll_upload(fftup_roll* r, const T** dptr, const std::vector<T>& h)
{
    void* d = nullptr;
    if (int rc = roll_alloc(r, &d, sizeof(T) * h.size())) return rc;
    HIP_TRY(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    *dptr = (const T*)d;
    return FFTUP_OK;
}

// exp(+i span k / m), k < m, in double, rounded once to fp32: span = 2 pi gives the m-th roots, span = pi the unit vectors of the
// polar grid's angles
std::vector<float2> phasors(uint32_t m, double span)
{
    std::vector<float2> h(m);
    for (uint32_t k = 0; k < m; k++) {
        const double t = span * (double)k / (double)m;
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

size_t rows_lds(const fftup_roll* r) { return 2 * sizeof(float2) * (size_t)lpad_size(2 * (int)r->g.nx); }
size_t cols_lds(const fftup_roll* r) { return 2 * sizeof(float2) * (size_t)lpad_size(4 * (int)r->g.ny); }
size_t polar_lds(const fftup_roll* r) { return 2 * sizeof(float2) * (size_t)lpad_size(2 * (int)r->g.ntheta); }
size_t peak_lds(const fftup_roll* r) { return 2 * sizeof(float2) * (size_t)lpad_size((int)r->g.ntheta); }

AlignImage image_of(const fftup_roll* r, const fftup_device_image& im)
{
    AlignImage q;
    q.data = (const uint8_t*)im.data;
    q.row = (long)im.row_stride_bytes;
    q.plane = (long)im.plane_stride_bytes;
    if (im.format == FFTUP_FMT_RGB8) q.kind = 0;
    else {
        const bool aligned = (uintptr_t)im.data % r->esz == 0;
        q.kind = r->esz == 4 ? (aligned ? 1 : 3) : (aligned ? 2 : 4);
    }
    return q;
}

}  // namespace

extern "C" {

int fftup_roll_create(fftup_roll** out, const fftup_roll_config* cfg)
{
    if (!out || !cfg) return fail(FFTUP_E_INVALID_ARG, "fftup_roll_create: null argument");
    *out = nullptr;
    RollGeometry G;
    if (int rc = roll_geometry(*cfg, G)) return rc;           // (before any device access)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); ndev = 0; }
    if (ndev <= 0) return fail(FFTUP_E_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(FFTUP_E_NO_DEVICE, "device id out of range");

    std::unique_ptr<fftup_roll, RollDestroyer> owner(new fftup_roll());
    fftup_roll* r = owner.get();
    r->g = G;
    r->device = cfg->device;
    r->esz = G.precision == 2 ? 2 : 4;
    r->thrX = fft_threads(2 * G.nx);
    r->thrY = fft_threads(4 * G.ny);
    r->thrT = fft_threads(2 * G.ntheta);
    HIP_TRY(hipSetDevice(r->device));
    RollParams& p = r->p;
    p.nx = (int)G.nx; p.ny = (int)G.ny; p.d = (int)G.d; p.crop_x = (int)G.crop_x; p.crop_y = (int)G.crop_y; p.kappa = (int)G.kappa;
    p.nt = (int)G.ntheta; p.rho_min = (int)G.rho_min; p.nrho = (int)(G.rho_max - G.rho_min + 1); p.mb = (int)G.mb;
    p.cx = (int)G.cx; p.cy = (int)G.cy; p.ncol = 2 * (int)G.cx + 3; p.nrow = (int)G.cy + 2;
    p.sx = (int)(G.nx / G.n); p.sy = (int)(G.ny / G.n);
    p.planX = make_stage_plan(2 * G.nx);
    p.planY = make_stage_plan(2 * G.ny);
    p.planT = make_stage_plan(G.ntheta);
    int rc;
    if ((rc = roll_upload(r, &p.twX, phasors(2 * G.nx, 2.0 * M_PI)))) return rc;
    if ((rc = roll_upload(r, &p.twY, phasors(2 * G.ny, 2.0 * M_PI)))) return rc;
    if ((rc = roll_upload(r, &p.twT, phasors(G.ntheta, 2.0 * M_PI)))) return rc;
    if ((rc = roll_upload(r, &p.winX, window(G.nx)))) return rc;
    if ((rc = roll_upload(r, &p.winY, window(G.ny)))) return rc;
    if ((rc = roll_upload(r, &p.cs, phasors(G.ntheta, M_PI)))) return rc;
    if ((rc = roll_upload(r, &p.ph, phasors(G.kappa * G.ntheta, 2.0 * M_PI)))) return rc;
    const size_t B = G.max_batch;
    if ((rc = roll_alloc(r, (void**)&p.Zr, sizeof(float2) * B * G.ny * p.ncol))) return rc;
    if ((rc = roll_alloc(r, (void**)&p.M, sizeof(float2) * B * p.nrow * p.ncol))) return rc;
    if ((rc = roll_alloc(r, (void**)&p.Pr, sizeof(float2) * B * p.nrho * G.mb))) return rc;
    *out = owner.release();
    return FFTUP_OK;
}

void fftup_roll_destroy(fftup_roll* r)
{
    if (!r) return;
    if (!r->allocs.empty()) {
        (void)hipSetDevice(r->device);
        (void)hipDeviceSynchronize();
        for (void* q : r->allocs) (void)hipFree(q);
    }
    delete r;
}

int fftup_roll_get_info(const fftup_roll* r, fftup_roll_info* info)
{
    if (!r || !info) return fail(FFTUP_E_INVALID_ARG, "fftup_roll_get_info: null argument");
    memset(info, 0, sizeof(*info));
    info->window_w = r->g.nx; info->window_h = r->g.ny; info->decimate = r->g.d;
    info->crop_x = r->g.crop_x; info->crop_y = r->g.crop_y; info->upsample = r->g.kappa;
    info->n = r->g.n; info->angles = r->g.ntheta; info->rho_min = r->g.rho_min; info->rho_max = r->g.rho_max;
    info->m_band = r->g.mb; info->K = r->g.K; info->max_batch = r->g.max_batch;
    info->num_kernels = NUM_KERNELS;
    info->device_bytes = r->device_bytes;
    for (int k = 0; k < NUM_KERNELS; k++) snprintf(info->kernel_names[k], sizeof(info->kernel_names[k]), "%s", KERNEL_NAMES[k]);
    return FFTUP_OK;
}

int fftup_roll_angles(fftup_roll* r, const fftup_device_image* ref, const fftup_device_image* cur, uint32_t n_pairs,
                      fftup_roll_angle* angles_device, void* stream)
{
    if (!r) return fail(FFTUP_E_INVALID_ARG, "fftup_roll_angles: null estimator");
    if (!ref || !cur) return fail(FFTUP_E_INVALID_ARG, "fftup_roll_angles: null image array");
    if (!angles_device) return fail(FFTUP_E_INVALID_ARG, "fftup_roll_angles: angles_device is null");
    if (n_pairs == 0) return fail(FFTUP_E_INVALID_ARG, "fftup_roll_angles: n_pairs must be > 0");
    HIP_TRY(hipSetDevice(r->device));
    // ---- everything that can be refused is refused here, before the first launch
    for (uint32_t i = 0; i < n_pairs; i++) {
        int rc = check_device_image(r->esz, false, r->device, ref[i], "ref", i, r->g.W, r->g.H, false);
        if (!rc) rc = check_device_image(r->esz, false, r->device, cur[i], "cur", i, r->g.W, r->g.H, false);
        if (rc) return rc;
    }
    if ((uintptr_t)angles_device % sizeof(float)) return fail(FFTUP_E_INVALID_ARG, "fftup_roll_angles: angles_device is not a multiple of 4 bytes");
    {
        hipPointerAttribute_t at{};
        const hipError_t e = hipPointerGetAttributes(&at, angles_device);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(FFTUP_E_INVALID_ARG, std::string("fftup_roll_angles: angles_device is not device memory (hipPointerGetAttributes: ") + hipGetErrorString(e) + ")");
        }
        if (at.type != hipMemoryTypeDevice || at.device != r->device)
            return fail(FFTUP_E_INVALID_ARG, "fftup_roll_angles: angles_device is not device memory of the estimator's device");
    }
    hipStream_t st = (hipStream_t)stream;
    const RollGeometry& g = r->g;
    const RollParams& p = r->p;
    for (uint32_t base = 0; base < n_pairs; base += g.max_batch) {       // a chunk reuses the buffers of the one before: stream order
        const uint32_t n = std::min(g.max_batch, n_pairs - base);
        for (uint32_t s = 0; s < n; s += ALIGN_PAIRS_PER_LAUNCH) {
            const uint32_t m = std::min<uint32_t>(ALIGN_PAIRS_PER_LAUNCH, n - s);
            AlignPairs q{};
            for (uint32_t k = 0; k < m; k++) {
                q.ref[k] = image_of(r, ref[base + s + k]);
                q.cur[k] = image_of(r, cur[base + s + k]);
            }
            hipLaunchKernelGGL(k_roll_rows, dim3(g.ny, 1, m), dim3(r->thrX), rows_lds(r), st, p, q, (int)s);
        }
        hipLaunchKernelGGL(k_roll_cols, dim3(g.cx + 2, 1, n), dim3(r->thrY), cols_lds(r), st, p);
        hipLaunchKernelGGL(k_roll_polar, dim3(p.nrho, 1, n), dim3(r->thrT), polar_lds(r), st, p);
        hipLaunchKernelGGL(k_roll_peak, dim3(1, 1, n), dim3(PEAK_THREADS), peak_lds(r), st, p, (float*)(angles_device + base));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(FFTUP_E_HIP, std::string("fftup_roll_angles: kernel launch: ") + hipGetErrorString(e));
    }
    return FFTUP_OK;
}

}  // extern "C"
