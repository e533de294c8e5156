// shift_path.hpp -- the arithmetic of fftup_shift_path (include/fftup.h, "a smoothed camera path"): measured shifts -> the camera
// path p -> its Gaussian low-pass s -> the view offsets p - s.  Plain C++ with __host__ __device__ functions when compiled as HIP;
// no HIP calls.  k_shift_path (kernels_path.hpp) and tests/path/shift_path_driver.cpp share every function here; tests/path_oracle.py
// restates the definition in numpy.
//
// Per axis, all in fp64, i = 0 .. n - 1:
//     frame i is MEASURED when peak >= min_peak (a NaN peak is not) and dx, dy are both finite
//     FFTUP_PATH_ABSOLUTE     p[i] = in[i] if measured, else p[i - 1];  p[-1] = 0
//     FFTUP_PATH_CONSECUTIVE  p[0] = 0 (in[0] is ignored), p[i] = p[i - 1] + in[i] if measured, else p[i - 1]
//     sigma == 0: s = 0.  Otherwise r = ceil(3 sigma), g[j] = exp(-j^2 / (2 sigma^2)),
//     s[i] = sum_{|j| <= r} g[j] p[clamp(i + j, 0, n - 1)] / sum_{|j| <= r} g[j],  both sums taken from j = -r upwards
//     out[i] = (float)(p[i] - s[i])
// Both modes are ONE prefix scan over elements (set, x, y) with the associative operator `join` below: a measured ABSOLUTE frame is
// (1, dx, dy) -- it replaces what came before; a measured CONSECUTIVE frame is (0, dx, dy) -- it adds to it; an unmeasured frame,
// and frame 0 of CONSECUTIVE, is (0, 0, 0).  p[i] = the inclusive scan's (x, y) at i.  The sums are of fp32 values in fp64.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FFTUP_PATH_HD __host__ __device__
#else
#define FFTUP_PATH_HD
#endif

namespace fftup_shiftpath {

constexpr uint32_t MODE_ABSOLUTE = 0, MODE_CONSECUTIVE = 1;
constexpr uint32_t MAX_FRAMES = 4096;
constexpr float MAX_SIGMA = 256.0f;
constexpr int MAX_RADIUS = 768;      // ceil(3 MAX_SIGMA)

struct Elem { int set; double x, y; };

FFTUP_PATH_HD inline bool measured(float dx, float dy, float peak, float min_peak)
{
    return peak >= min_peak && std::isfinite(dx) && std::isfinite(dy);          // (NaN >= anything: false)
}

// what frame i brings to the scan (the increment / hold rule)
FFTUP_PATH_HD inline Elem elem_of(uint32_t mode, uint32_t i, float dx, float dy, float peak, float min_peak)
{
    if (!measured(dx, dy, peak, min_peak) || (mode == MODE_CONSECUTIVE && i == 0)) return {0, 0.0, 0.0};
    return {mode == MODE_ABSOLUTE ? 1 : 0, (double)dx, (double)dy};
}

// a then b (associative; the identity is (0, 0, 0))
FFTUP_PATH_HD inline Elem join(const Elem& a, const Elem& b)
{
    if (b.set) return b;
    return {a.set, a.x + b.x, a.y + b.y};
}

FFTUP_PATH_HD inline int radius_of(double sigma) { return sigma > 0.0 ? (int)std::ceil(3.0 * sigma) : 0; }

// g[j], sigma > 0
FFTUP_PATH_HD inline double weight_of(int j, double sigma)
{
    const double t = (double)j;
    return std::exp(-(t * t) / (2.0 * sigma * sigma));
}

FFTUP_PATH_HD inline int clamp_index(int k, int n) { return k < 0 ? 0 : (k >= n ? n - 1 : k); }

// s[i] of one axis: p(k) the path at k in [0, n), g(j) the weight at j in [0, r]
template <class PathAt, class WeightAt> FFTUP_PATH_HD inline double smoothed_at(PathAt p, WeightAt g, int i, int n, int r)
{
    double acc = 0.0, norm = 0.0;
    for (int j = -r; j <= r; j++) {
        const double w = g(j < 0 ? -j : j);
        const double term = w * p(clamp_index(i + j, n));
        acc += term;
        norm += w;
    }
    return acc / norm;
}

}  // namespace fftup_shiftpath
