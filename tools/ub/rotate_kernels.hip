// rotate_kernels.hip -- device time of each of the rotator's three kernels (csrc/kernels_rotate.hpp), a pair of events around every
// launch on one stream: what fftup_rotate_frames enqueues for a chunk, kernel by kernel.  A record, not a gate (tools/rotate_time.py
// runs it and files the figures).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=on -I vkresample_amd/csrc tools/ub/rotate_kernels.hip -o tools/ub/rotate_kernels
//   tools/ub/rotate_kernels W H [frames = 16] [rounds = 8] [kind = 0 (8-bit frames) | 1 (float planes)] [row threads] [column threads]
// (the thread counts default to the library's; multiples of 64 up to 1024 otherwise)
// prints one JSON object: us per frame and kernel, medians of `rounds` rounds after one warm-up round, with min and max.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels_rotate.hpp"

using namespace fftup;

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        const hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

// the radix sequence of plan_rules.cpp (make_stage_plan): 8s, then 4 or 2, then 3, 5, 7
static bool stage_plan(uint32_t n, StagePlan& p)
{
    p = StagePlan{};
    p.n = (int)n;
    uint32_t m = n;
    int e2 = 0, ns = 0;
    while (m % 2 == 0) { m /= 2; e2++; }
    while (e2 >= 3) { p.radix[ns++] = 8; e2 -= 3; }
    if (e2 == 2) p.radix[ns++] = 4;
    if (e2 == 1) p.radix[ns++] = 2;
    for (uint32_t q : {3u, 5u, 7u})
        while (m % q == 0) { p.radix[ns++] = (uint8_t)q; m /= q; }
    p.nstages = ns;
    return m == 1 && n >= 2 && n <= 4096;
}

static int roots(const float2** d, uint32_t n)
{
    std::vector<float2> h(n);
    for (uint32_t k = 0; k < n; k++) h[k] = make_float2((float)std::cos(2.0 * M_PI * k / n), (float)std::sin(2.0 * M_PI * k / n));
    CHECK(hipMalloc((void**)d, sizeof(float2) * n));
    CHECK(hipMemcpy((void*)*d, h.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
    return 0;
}

static int threads(size_t points) { return points <= 512 ? 64 : points <= 2048 ? 128 : 256; }

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: rotate_kernels W H [frames] [rounds] [kind]\n"); return 2; }
    const uint32_t W = (uint32_t)atoi(argv[1]), H = (uint32_t)atoi(argv[2]);
    const int frames = argc > 3 ? atoi(argv[3]) : 16, rounds = argc > 4 ? atoi(argv[4]) : 8, kind = argc > 5 ? atoi(argv[5]) : 0;
    RotateParams p{};
    p.W = (int)W; p.H = (int)H;
    if (!stage_plan(W, p.planW) || !stage_plan(H, p.planH) || frames < 1 || frames > ROTATE_FRAMES_PER_LAUNCH || rounds < 1 || (kind != 0 && kind != 1)) {
        fprintf(stderr, "W and H: 2,3,5,7-smooth in [2, 4096]; frames in [1, %d]; kind 0 or 1\n", ROTATE_FRAMES_PER_LAUNCH);
        return 2;
    }
    const uint32_t TK = 2 * H <= 4096 ? 4 : 2;
    const size_t lds_x = 2 * sizeof(float2) * (size_t)lpad_size(2 * (int)W), lds_y = 2 * sizeof(float2) * (size_t)lpad_size((int)(TK * H));
    if (roots(&p.twW, W) || roots(&p.twH, H)) return 1;
    const size_t px = (size_t)frames * W * H, frame_bytes = (size_t)W * H * (kind ? 12 : 3);
    CHECK(hipMalloc((void**)&p.rg1, sizeof(float2) * px));
    CHECK(hipMalloc((void**)&p.rg2, sizeof(float2) * px));
    CHECK(hipMalloc((void**)&p.b1, sizeof(float) * px));
    CHECK(hipMalloc((void**)&p.b2, sizeof(float) * px));
    uint8_t *din = nullptr, *dout = nullptr;
    CHECK(hipMalloc((void**)&din, frame_bytes * frames));
    CHECK(hipMalloc((void**)&dout, frame_bytes * frames));
    CHECK(hipMemset(din, 0x40, frame_bytes * frames));
    RotateFrames q{};
    for (int k = 0; k < frames; k++) {
        const long row = kind ? 4l * W : 3l * W, plane = kind ? 4l * W * H : 0;
        q.in[k] = RotateImage{din + frame_bytes * k, row, plane, kind};
        q.out[k] = RotateImage{dout + frame_bytes * k, row, plane, kind};
        const double theta = 0.02 + 0.01 * k;
        q.a[k] = fftup_rotphase::shear_a(theta); q.b[k] = fftup_rotphase::shear_b(theta);
        q.cx[k] = 0.5 * (W - 1); q.cy[k] = 0.5 * (H - 1);
    }
    auto shear_y = TK == 4 ? k_rotate_shear_y<4> : k_rotate_shear_y<2>;
    CHECK(hipFuncSetAttribute((const void*)k_rotate_shear_x<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_x));
    CHECK(hipFuncSetAttribute((const void*)k_rotate_shear_x<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_x));
    CHECK(hipFuncSetAttribute((const void*)shear_y, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_y));
    hipStream_t st;
    CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipEvent_t ev[4];
    for (auto& e : ev) CHECK(hipEventCreate(&e));
    const int thrX = argc > 6 ? atoi(argv[6]) : threads(2 * (size_t)W), thrY = argc > 7 ? atoi(argv[7]) : threads((size_t)TK * H);
    if (thrX < 64 || thrX > 1024 || thrX % 64 || thrY < 64 || thrY > 1024 || thrY % 64) { fprintf(stderr, "thread counts: multiples of 64 up to 1024\n"); return 2; }
    std::vector<float> t[3];
    for (int r = 0; r <= rounds; r++) {                      // (round 0 warms up)
        CHECK(hipEventRecord(ev[0], st));
        hipLaunchKernelGGL(k_rotate_shear_x<0>, dim3(H, 1, frames), dim3(thrX), lds_x, st, p, q, 0, (const double2*)nullptr);
        CHECK(hipEventRecord(ev[1], st));
        hipLaunchKernelGGL(shear_y, dim3((W + TK - 1) / TK, 2, frames), dim3(thrY), lds_y, st, p, q, 0, (const double2*)nullptr);
        CHECK(hipEventRecord(ev[2], st));
        hipLaunchKernelGGL(k_rotate_shear_x<1>, dim3(H, 1, frames), dim3(thrX), lds_x, st, p, q, 0, (const double2*)nullptr);
        CHECK(hipEventRecord(ev[3], st));
        CHECK(hipGetLastError());
        CHECK(hipEventSynchronize(ev[3]));
        for (int k = 0; k < 3 && r; k++) {
            float ms = 0;
            CHECK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
            t[k].push_back(ms * 1e3f / (float)frames);
        }
    }
    const char* names[3] = {"rotate_shear_x_in", "rotate_shear_y", "rotate_shear_x_out"};
    printf("{\"size\": \"%ux%u\", \"kind\": \"%s\", \"frames_per_launch\": %d, \"rounds\": %d, \"column_tile\": %u, \"threads\": [%d, %d, %d], \"lds_bytes\": [%zu, %zu, %zu], \"us_per_frame\": {",
           W, H, kind ? "planar_f32" : "rgb8", frames, rounds, TK, thrX, thrY, thrX, lds_x, lds_y, lds_x);
    for (int k = 0; k < 3; k++) {
        std::sort(t[k].begin(), t[k].end());
        const size_t n = t[k].size();
        const float med = n % 2 ? t[k][n / 2] : 0.5f * (t[k][n / 2 - 1] + t[k][n / 2]);
        printf("%s\"%s\": {\"median\": %.2f, \"min_max\": [%.2f, %.2f]}", k ? ", " : "", names[k], med, t[k].front(), t[k].back());
    }
    printf("}}\n");
    return 0;
}
