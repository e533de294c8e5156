// kernels_view_tables.hpp -- k_view_tables: the chirp tables of a view (kernels_view.hpp: pre, post, bhat) built on the device, for
// the frames of fftup_execute_device_views, each of which brings its own view.  The host path of fftup_plan_set_view
// (view_tables.hpp: long double phases, a recursive fp64 FFT, blocking copies) stays what it is; this kernel is enqueued on the
// frame's lane stream ahead of the frame's four kernels, so stream order alone keeps the tables whole: the lane's next frame
// rebuilds them behind this frame's last reader.
//
// One workgroup per axis (grid 2).  The phases are view_phase.hpp's -- fp64, compensated, reduced modulo 2 before the
// multiplication by pi -- and every entry is rounded to fp32 once.  bhat = FFT_L(c wrapped) / L: the chirp is formed in fp64 in
// LDS and transformed there in fp64 by the in-place Stockham stages of fft_engine.hpp with exp(+2 pi i nk / L), as host_fft does,
// then rounded once.  LDS: ONE double2 buffer of lpad_size(L) points -- the bytes of the two float2 buffers the view kernels need
// for the same L, so every L a view plan accepts fits.  The in-place stages keep a thread's points in registers:
// fft_lds_inplace<+1, VT_PT> on VT_THREADS threads holds every smooth L up to 14336 (stage_fits_inplace; the radix-7 stage is the
// tightest), above the 9637 points that fit the LDS.  The fp64 L-th roots are a table per axis the plan uploads once.
// A pan (chirp == 0) rebuilds `pre` alone, the one table the origin enters.
// fftup_execute_device_views_shifted: the origin is moved by a float the kernel reads from device memory when it runs -- the host
// never sees it; everything else about the frame depends on the span alone and stays the host's.
#pragma once
#include <hip/hip_runtime.h>

#include "fft_engine.hpp"
#include "view_phase.hpp"

namespace fftup {

constexpr int VT_THREADS = 1024;     // one workgroup of 16 waves
constexpr int VT_PT = 16;            // points a thread holds across the barrier of an in-place stage
constexpr int VT_MAX_L = 14336;      // stage_fits_inplace(L, R, VT_THREADS, VT_PT) for R = 2, 3, 4, 5, 7, 8 up to here

struct ViewTabAxis {
    int32_t n, M, L;         // the period (the input length, doubled for a mirror axis), points out, convolution length
    int32_t kmax;
    int32_t chirp;           // 0: only `pre` is written
    double o_hi, o_lo, span; // the origin modulo n (mirror: + 1/2) as a pair (fftup_viewphase::origin_of, on the host)
    // fftup_execute_device_views_shifted: the axis' float of the frame's fftup_shift in device memory (nullptr: none, o_hi / o_lo
    // hold) -- the kernel moves `origin` by it and forms the pair itself, with the function the host forms o_hi / o_lo with
    double origin;           // the view's origin as the caller gave it
    int32_t mirror;
    const float* shift;
    StagePlan plan;          // n = L
    const double2* tw;       // L-th roots in double, exp(+2 pi i k / L)
    float2* pre;             // 2 kmax + 1 points
    float2* post;            // M points
    float2* bhat;            // L points
};
struct ViewTabParams { ViewTabAxis ax[2]; };

// grid (2); block VT_THREADS; dynamic LDS = sizeof(double2) * lpad_size(max L)
__global__ void __launch_bounds__(VT_THREADS) k_view_tables(ViewTabParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* c = (double2*)smem;
    const ViewTabAxis& x = p.ax[blockIdx.x];
    const int tid = threadIdx.x, T = blockDim.x;
    fftup_viewphase::Pair o{x.o_hi, x.o_lo};
    if (x.shift) {                                             // (workgroup-uniform; a shift that is not finite counts as 0)
        const float d = *x.shift;
        o = fftup_viewphase::origin_of(x.origin + (std::isfinite(d) ? (double)d : 0.0), (double)x.n, x.mirror != 0);
    }
    const fftup_viewphase::Axis a = fftup_viewphase::axis_of((uint32_t)x.n, (uint32_t)x.M, o, x.span, x.kmax);
    const int K = 2 * x.kmax + 1;
    for (int j = tid; j < K; j += T) {
        const fftup_viewphase::Cplx w = fftup_viewphase::pre_of(a, j);
        x.pre[j] = make_float2((float)w.re, (float)w.im);
    }
    if (!x.chirp) return;                                      // (workgroup-uniform)
    for (int m = tid; m < x.M; m += T) {
        const fftup_viewphase::Cplx w = fftup_viewphase::post_of(a, m);
        x.post[m] = make_float2((float)w.re, (float)w.im);
    }
    const int L = x.L;
    for (int i = tid; i < L; i += T) {
        const fftup_viewphase::Cplx w = fftup_viewphase::chirp_wrapped(a, i, L);
        c[lpad(i)] = make_double2(w.re, w.im);
    }
    __syncthreads();
    fft_lds_inplace<+1, VT_PT>(c, x.plan, x.tw, tid, T);
    for (int k = tid; k < L; k += T) {
        const double2 v = c[lpad(k)];
        x.bhat[k] = make_float2((float)(v.x / (double)L), (float)(v.y / (double)L));       // (divided, as make_axis does)
    }
}

}  // namespace fftup
