// kernels_path.hpp -- k_shift_path: fftup_shift_path on the device, the arithmetic of shift_path.hpp.  ONE workgroup (n is at most
// FFTUP_PATH_MAX_FRAMES = 4096): thread t owns the frames [4 t, 4 t + 4).
//   1. every thread reads its frames' fftup_shift into registers and scans them serially -- these are the kernel's only reads of
//      `in`, and they all come before the first barrier, the kernel's stores all behind the second: out == in is safe
//   2. the threads' totals are scanned across the wave by __shfl_up, the waves' totals through LDS; p[i] goes to LDS as an fp64 pair
//   3. behind a barrier every thread forms the clamped window sums of its frames from LDS (the weights g[0 .. r] are a table there)
//      and stores dx, dy = (float)(p - s) with the frame's peak and peak_coarse as it read them
// No atomics: the same call gives the same bytes.  Dynamic LDS: shift_path_lds(n, r) -- 64 KB of path at n = 4096 plus the weights
// and the waves' totals, above the 64 KB a kernel gets unasked (launch_shift_path allows it).
#pragma once
#include <hip/hip_runtime.h>

#include "shift_path.hpp"

namespace fftup {

constexpr int SP_THREADS = 1024;     // 16 waves
constexpr int SP_PER_THREAD = 4;     // SP_THREADS * SP_PER_THREAD = FFTUP_PATH_MAX_FRAMES
constexpr int SP_WAVES = SP_THREADS / 64;
static_assert((uint32_t)(SP_THREADS * SP_PER_THREAD) == fftup_shiftpath::MAX_FRAMES, "one workgroup holds the longest path");

struct ShiftPathParams {
    const float* in;         // n fftup_shift: dx, dy, peak, peak_coarse
    float* out;              // n fftup_shift (may be `in`)
    int32_t n;
    uint32_t mode;
    float sigma, min_peak;
};

// double2 p[n] | double g[r + 1] | double wx[SP_WAVES], wy[SP_WAVES] | int wset[SP_WAVES]
inline size_t shift_path_lds(int n, int r)
{
    return sizeof(double2) * (size_t)n + sizeof(double) * (size_t)(r + 1) + (2 * sizeof(double) + sizeof(int)) * SP_WAVES;
}

// grid (1); block SP_THREADS; dynamic LDS = shift_path_lds(n, radius_of(sigma))
__global__ void __launch_bounds__(SP_THREADS) k_shift_path(ShiftPathParams q)
{
    namespace sp = fftup_shiftpath;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = q.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double sigma = (double)q.sigma;
    const int r = sp::radius_of(sigma);
    double2* p = (double2*)smem;
    double* g = (double*)(p + n);
    double* wx = g + (r + 1);
    double* wy = wx + SP_WAVES;
    int* wset = (int*)(wy + SP_WAVES);

    // 1. this thread's frames: read once, scanned serially (e[k]: the scan of the thread's frames up to k)
    float peak[SP_PER_THREAD], coarse[SP_PER_THREAD];
    sp::Elem e[SP_PER_THREAD];
    sp::Elem run{0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < SP_PER_THREAD; k++) {
        const int i = SP_PER_THREAD * tid + k;
        peak[k] = coarse[k] = 0.f;
        if (i < n) {
            const float dx = q.in[4 * i], dy = q.in[4 * i + 1];
            peak[k] = q.in[4 * i + 2]; coarse[k] = q.in[4 * i + 3];
            run = sp::join(run, sp::elem_of(q.mode, (uint32_t)i, dx, dy, peak[k], q.min_peak));
        }
        e[k] = run;
    }
    for (int j = tid; j <= r; j += SP_THREADS) g[j] = r ? sp::weight_of(j, sigma) : 1.0;

    // 2. the threads' totals across the wave (inclusive), the waves' totals through LDS
    sp::Elem t = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const sp::Elem u{__shfl_up(t.set, o), __shfl_up(t.x, o), __shfl_up(t.y, o)};
        if (lane >= o) t = sp::join(u, t);
    }
    sp::Elem before{__shfl_up(t.set, 1), __shfl_up(t.x, 1), __shfl_up(t.y, 1)};      // the wave's threads ahead of this one
    if (lane == 0) before = {0, 0.0, 0.0};
    if (lane == 63) { wx[wave] = t.x; wy[wave] = t.y; wset[wave] = t.set; }
    __syncthreads();
    sp::Elem base{0, 0.0, 0.0};
    for (int w = 0; w < wave; w++) base = sp::join(base, {wset[w], wx[w], wy[w]});
    base = sp::join(base, before);
#pragma unroll
    for (int k = 0; k < SP_PER_THREAD; k++) {
        const int i = SP_PER_THREAD * tid + k;
        e[k] = sp::join(base, e[k]);
        if (i < n) p[i] = make_double2(e[k].x, e[k].y);
    }
    __syncthreads();

    // 3. the window sums and the offsets
#pragma unroll
    for (int k = 0; k < SP_PER_THREAD; k++) {
        const int i = SP_PER_THREAD * tid + k;
        if (i >= n) continue;
        double sx = 0.0, sy = 0.0;
        if (r) {
            const auto weight = [&](int j) { return g[j]; };
            sx = sp::smoothed_at([&](int m) { return p[m].x; }, weight, i, n, r);
            sy = sp::smoothed_at([&](int m) { return p[m].y; }, weight, i, n, r);
        }
        q.out[4 * i] = (float)(e[k].x - sx);
        q.out[4 * i + 1] = (float)(e[k].y - sy);
        q.out[4 * i + 2] = peak[k];
        q.out[4 * i + 3] = coarse[k];
    }
}

}  // namespace fftup
