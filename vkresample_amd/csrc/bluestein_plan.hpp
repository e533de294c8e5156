// bluestein_plan.hpp -- how ONE 1-D transform of a plan runs (FFTUP_FLAG_ANY_SIZE, include/fftup.h): directly, by the Stockham
// stages of its own StagePlan (L = 0: the length is 2,3,5,7-smooth), or as a chirp-z (Bluestein) transform through two transforms
// of a smooth length L >= 2N - 1 (kernels_bluestein.hpp).  Shared by the planner (plan.hpp) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_engine.hpp"

namespace fftup {

struct BzPlan {
    int32_t L;               // 0: direct transform; else the Bluestein length (smooth, >= 2N - 1, two LDS buffers of L * TK points fit)
    StagePlan plan;          // n = L
    const float2* tw;        // L-th roots, exp(+2 pi i k / L)
    const float2* chirp;     // exp(+i pi n^2 / N), n < N
    const float2* bhat;      // FFT_L(conj chirp, wrapped to [-(N-1), N-1]) / L, L points
};

}  // namespace fftup
