// fftup_rotate.hip -- rotation by three shears: the rotator object of include/fftup.h (fftup_rotate_create / _destroy / _get_info /
// _frames / _frames_angles) and the launches of its kernels (kernels_rotate.hpp).  The geometry comes from rotate_geometry (plan_rules.cpp), before
// any device access; the twiddle tables and the two fp32 intermediates of max_batch frames are made at creation, where the
// kernels are also allowed their dynamic LDS; fftup_rotate_frames validates, then only launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "kernels_rotate.hpp"
#include "plan.hpp"

using namespace fftup;

struct fftup_rotate {
    RotateGeometry g;
    int device = 0;
    size_t esz = 4;                   // bytes of a FFTUP_FMT_PLANAR element
    RotateParams p{};
    int thrX = 64, thrY = 64;         // threads of the row kernels / the column kernel
    double2* coef = nullptr;          // [max_batch]: the shear coefficients (a, b) of a chunk, fftup_rotate_frames_angles
    std::vector<void*> allocs;
    uint64_t device_bytes = 0;
};

namespace {

const char* const KERNEL_NAMES[] = {"rotate_shear_x_in", "rotate_shear_y", "rotate_shear_x_out"};
constexpr int NUM_KERNELS = 3;

struct RotateDestroyer { void operator()(fftup_rotate* r) const { fftup_rotate_destroy(r); } };

int rotate_alloc(fftup_rotate* r, void** ptr, size_t bytes)
{
    const hipError_t e = hipMalloc(ptr, bytes);
    if (e != hipSuccess) {
        *ptr = nullptr;
        (void)hipGetLastError();
        return fail(FFTUP_E_OUT_OF_MEMORY, std::string("fftup_rotate_create: hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    }
    r->allocs.push_back(*ptr);
    r->device_bytes += bytes;
    return FFTUP_OK;
}

// the n-th roots exp(+2 pi i k / n) in double, rounded once to fp32
int rotate_roots(fftup_rotate* r, const float2** dptr, uint32_t n)
{
    std::vector<float2> h(n);
    for (uint32_t k = 0; k < n; k++) {
        const double t = 2.0 * M_PI * (double)k / (double)n;
        h[k] = make_float2((float)std::cos(t), (float)std::sin(t));
    }
    void* d = nullptr;
    if (int rc = rotate_alloc(r, &d, sizeof(float2) * n)) return rc;
    HIP_TRY(hipMemcpy(d, h.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
    *dptr = (const float2*)d;
    return FFTUP_OK;
}

// threads for `points` complex points in LDS (a radix-8 butterfly takes eight of them)
int fft_threads(size_t points) { return points <= 512 ? 64 : points <= 2048 ? 128 : 256; }

RotateImage image_of(const fftup_rotate* r, const fftup_device_image& im)
{
    RotateImage q;
    q.data = (uint8_t*)im.data;
    q.row = (long)im.row_stride_bytes;
    q.plane = (long)im.plane_stride_bytes;
    if (im.format == FFTUP_FMT_RGB8) q.kind = 0;
    else {
        const bool aligned = (uintptr_t)im.data % r->esz == 0;
        q.kind = r->esz == 4 ? (aligned ? 1 : 3) : (aligned ? 2 : 4);
    }
    return q;
}

using ShearY = void (*)(RotateParams, RotateFrames, int, const double2*);
ShearY shear_y_kernel(const fftup_rotate* r) { return r->g.TK == 4 ? k_rotate_shear_y<4> : k_rotate_shear_y<2>; }

// Both entry points: validation, then the launches.  angles == nullptr: fftup_rotate_frames, the coefficients travel in the kernel
// arguments; otherwise one k_rotate_coeffs per chunk fills r->coef from the device angles and the shear kernels read them there
int rotate_run(const char* who_c, fftup_rotate* r, const fftup_device_image* in, const fftup_device_image* out, const fftup_rotation* rotations,
               const fftup_roll_angle* angles, double gain, uint32_t n_frames, void* stream)
{
    const std::string who = who_c;
    if (!r) return fail(FFTUP_E_INVALID_ARG, who + "null rotator");
    if (!in || !out) return fail(FFTUP_E_INVALID_ARG, who + "null image array");
    if (!rotations) return fail(FFTUP_E_INVALID_ARG, who + "rotations is null");
    if (n_frames == 0) return fail(FFTUP_E_INVALID_ARG, who + "n_frames must be > 0");
    HIP_TRY(hipSetDevice(r->device));
    // ---- everything that can be refused is refused here, before the first launch
    for (uint32_t i = 0; i < n_frames; i++) {
        const fftup_rotation& t = rotations[i];
        const std::string at = who + "rotations[" + std::to_string(i) + "]";
        if (!std::isfinite(t.angle)) return fail(FFTUP_E_INVALID_ARG, at + ".angle is not finite");
        if (!std::isfinite(t.centre_x) || !std::isfinite(t.centre_y)) return fail(FFTUP_E_INVALID_ARG, at + ": the centre is not finite");
        if (std::fabs(t.angle) > M_PI / 2) return fail(FFTUP_E_INVALID_ARG, at + ".angle is beyond pi / 2 in magnitude (transpose or flip first)");
        int rc = check_device_image(r->esz, false, r->device, in[i], "in", i, r->g.W, r->g.H, false);
        if (!rc) rc = check_device_image(r->esz, false, r->device, out[i], "out", i, r->g.W, r->g.H, true);
        if (rc) return rc;
    }
    if (angles) {
        hipPointerAttribute_t at{};
        const hipError_t e = hipPointerGetAttributes(&at, angles);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(FFTUP_E_INVALID_ARG, who + "angles_device is not device memory (hipPointerGetAttributes: " + hipGetErrorString(e) + ")");
        }
        if (at.type != hipMemoryTypeDevice || at.device != r->device)
            return fail(FFTUP_E_INVALID_ARG, who + "angles_device is not device memory of the rotator's device");
    }
    hipStream_t st = (hipStream_t)stream;
    const RotateGeometry& g = r->g;
    const RotateParams& p = r->p;
    const ShearY shear_y = shear_y_kernel(r);
    const uint32_t tiles = (g.W + g.TK - 1) / g.TK;
    const double2* coef = angles ? r->coef : nullptr;
    for (uint32_t base = 0; base < n_frames; base += g.max_batch) {      // a chunk reuses the intermediates of the one before: stream order
        const uint32_t n = std::min(g.max_batch, n_frames - base);
        if (angles) {
            RotateHostAngles h{};
            for (uint32_t k = 0; k < n; k++) h.angle[k] = rotations[base + k].angle;
            hipLaunchKernelGGL(k_rotate_coeffs, dim3(1), dim3(ROTATE_MAX_BATCH), 0, st, h, (const float*)(angles + base), gain, (int)n, r->coef);
        }
        for (int pass = 0; pass < 3; pass++)
            for (uint32_t s = 0; s < n; s += ROTATE_FRAMES_PER_LAUNCH) {
                const uint32_t m = std::min<uint32_t>(ROTATE_FRAMES_PER_LAUNCH, n - s);
                RotateFrames q{};
                for (uint32_t k = 0; k < m; k++) {
                    const fftup_rotation& t = rotations[base + s + k];
                    q.in[k] = image_of(r, in[base + s + k]);
                    q.out[k] = image_of(r, out[base + s + k]);
                    // the coefficients in the arguments are the host path's; with device angles the kernels read `coef` and
                    // these stay 0, so that nothing in a launch suggests a rotation by the host angle alone
                    q.a[k] = coef ? 0.0 : fftup_rotphase::shear_a(t.angle);
                    q.b[k] = coef ? 0.0 : fftup_rotphase::shear_b(t.angle);
                    q.cx[k] = t.centre_x;
                    q.cy[k] = t.centre_y;
                }
                if (pass == 0) hipLaunchKernelGGL(k_rotate_shear_x<0>, dim3(g.H, 1, m), dim3(r->thrX), g.lds_x, st, p, q, (int)s, coef);
                else if (pass == 1) hipLaunchKernelGGL(shear_y, dim3(tiles, 2, m), dim3(r->thrY), g.lds_y, st, p, q, (int)s, coef);
                else hipLaunchKernelGGL(k_rotate_shear_x<1>, dim3(g.H, 1, m), dim3(r->thrX), g.lds_x, st, p, q, (int)s, coef);
            }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(FFTUP_E_HIP, who + "kernel launch: " + hipGetErrorString(e));
    }
    return FFTUP_OK;
}

}  // namespace

extern "C" {

int fftup_rotate_create(fftup_rotate** out, const fftup_rotate_config* cfg)
{
    if (!out || !cfg) return fail(FFTUP_E_INVALID_ARG, "fftup_rotate_create: null argument");
    *out = nullptr;
    RotateGeometry G;
    if (int rc = rotate_geometry(*cfg, G)) return rc;         // (before any device access)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); ndev = 0; }
    if (ndev <= 0) return fail(FFTUP_E_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(FFTUP_E_NO_DEVICE, "device id out of range");

    std::unique_ptr<fftup_rotate, RotateDestroyer> owner(new fftup_rotate());
    fftup_rotate* r = owner.get();
    r->g = G;
    r->device = cfg->device;
    r->esz = G.precision == 2 ? 2 : 4;
    r->thrX = fft_threads(2 * (size_t)G.W);
    r->thrY = fft_threads((size_t)G.TK * G.H);
    HIP_TRY(hipSetDevice(r->device));
    RotateParams& p = r->p;
    p.W = (int)G.W; p.H = (int)G.H;
    p.planW = make_stage_plan(G.W);
    p.planH = make_stage_plan(G.H);
    int rc;
    if ((rc = rotate_roots(r, &p.twW, G.W))) return rc;
    if ((rc = rotate_roots(r, &p.twH, G.H))) return rc;
    const size_t px = (size_t)G.max_batch * G.W * G.H;
    if ((rc = rotate_alloc(r, (void**)&p.rg1, sizeof(float2) * px))) return rc;
    if ((rc = rotate_alloc(r, (void**)&p.rg2, sizeof(float2) * px))) return rc;
    if ((rc = rotate_alloc(r, (void**)&p.b1, sizeof(float) * px))) return rc;
    if ((rc = rotate_alloc(r, (void**)&p.b2, sizeof(float) * px))) return rc;
    if ((rc = rotate_alloc(r, (void**)&r->coef, sizeof(double2) * G.max_batch))) return rc;
    // dynamic LDS above 64 KB needs the attribute
    const struct { const void* fn; size_t lds; } kerns[3] = {{(const void*)k_rotate_shear_x<0>, G.lds_x}, {(const void*)shear_y_kernel(r), G.lds_y},
                                                              {(const void*)k_rotate_shear_x<1>, G.lds_x}};
    for (const auto& k : kerns) {
        const hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds);
        if (e != hipSuccess) return fail(FFTUP_E_HIP, std::string("fftup_rotate_create: hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize): ") + hipGetErrorString(e));
    }
    *out = owner.release();
    return FFTUP_OK;
}

void fftup_rotate_destroy(fftup_rotate* r)
{
    if (!r) return;
    if (!r->allocs.empty()) {
        (void)hipSetDevice(r->device);
        (void)hipDeviceSynchronize();
        for (void* q : r->allocs) (void)hipFree(q);
    }
    delete r;
}

int fftup_rotate_get_info(const fftup_rotate* r, fftup_rotate_info* info)
{
    if (!r || !info) return fail(FFTUP_E_INVALID_ARG, "fftup_rotate_get_info: null argument");
    memset(info, 0, sizeof(*info));
    info->width = r->g.W; info->height = r->g.H; info->max_batch = r->g.max_batch;
    info->num_kernels = NUM_KERNELS;
    info->device_bytes = r->device_bytes;
    for (int k = 0; k < NUM_KERNELS; k++) snprintf(info->kernel_names[k], sizeof(info->kernel_names[k]), "%s", KERNEL_NAMES[k]);
    return FFTUP_OK;
}

int fftup_rotate_frames(fftup_rotate* r, const fftup_device_image* in, const fftup_device_image* out, const fftup_rotation* rotations,
                        uint32_t n_frames, void* stream)
{
    return rotate_run("fftup_rotate_frames: ", r, in, out, rotations, nullptr, 0.0, n_frames, stream);
}

int fftup_rotate_frames_angles(fftup_rotate* r, const fftup_device_image* in, const fftup_device_image* out, const fftup_rotation* rotations,
                               const fftup_roll_angle* angles_device, double gain, uint32_t n_frames, void* stream)
{
    const std::string who = "fftup_rotate_frames_angles: ";
    if (!angles_device) return fail(FFTUP_E_INVALID_ARG, who + "angles_device is null");
    if (!std::isfinite(gain)) return fail(FFTUP_E_INVALID_ARG, who + "gain is not finite");
    if ((uintptr_t)angles_device % sizeof(float)) return fail(FFTUP_E_INVALID_ARG, who + "angles_device is not a multiple of 4 bytes");
    return rotate_run(who.c_str(), r, in, out, rotations, angles_device, gain, n_frames, stream);
}

}  // extern "C"
