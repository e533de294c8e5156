// kernels_rotate.hpp -- rotation by three shears (include/fftup.h, fftup_rotate_frames): R(theta) = Sx(a) Sy(b) Sx(a) with
// a = -tan(theta / 2), b = sin(theta).  A shear moves every row (column) by its own sub-pixel amount delta: forward transform in
// LDS, one complex multiply per bin (rotate_phase.hpp: the phase formed and reduced in double), inverse transform, times 1/n.
// Three launches per chunk of frames, the frame in blockIdx.z, its descriptors and coefficients in the kernel arguments (the
// coefficients in a device buffer that k_rotate_coeffs fills first when the angles come from device memory):
//   k_rotate_shear_x<0>  one workgroup per row: the caller's frame (any of the five kinds of RotateImage) -> T1
//   k_rotate_shear_y<TK> one workgroup per tile of TK adjacent columns of ONE of the two sequences (blockIdx.y): T1 -> T2; every
//                        column has its own delta; the last tile of a width that is no multiple of TK is partial
//   k_rotate_shear_x<1>  one workgroup per row: T2 -> the caller's frame, format and strides (planes: one rounding from fp32;
//                        8-bit: clamp(floor(255 x + 0.5)))
// The three planes ride two complex sequences: z0 = R + i G and z1 = B + i 0.  The operator of a shear is real and linear (the
// factors of bins f and -f are conjugates, the Nyquist factor is real), so z0 times the factors is exact for both planes: no
// separation step.  What the rounding leaves in Im z1 is dropped.  The intermediates hold z0 as float2 [frame][H][W] and B as
// float [frame][H][W]; they are fp32 for every input format.
// Transform direction: fft_engine's DIR = -1 is numpy's forward DFT.  LDS: two buffers of two interleaved sequences of W points
// for the rows, of TK interleaved columns of H points for the columns -- 2 * lpad_size(8192) * 8 B = 139 280 B at the longest
// lengths (W = 4096; H = 2048 with TK = 4, H = 4096 with TK = 2).  Not handed to the plan-time compiler.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_engine.hpp"
#include "rotate_phase.hpp"

namespace fftup {

// one frame, as the aligner's AlignImage: kind 0 RGB8, 1 float planes, 2 half planes, 3 / 4 the same planes at an address that is no
// multiple of the element size (assembled from and taken apart into bytes); strides in bytes
struct RotateImage { uint8_t* data; long row, plane; int kind; };
constexpr int ROTATE_FRAMES_PER_LAUNCH = 16;     // descriptors travel as kernel arguments: read before the launch returns
// the frames of one launch: images, shear coefficients and centres
struct RotateFrames {
    RotateImage in[ROTATE_FRAMES_PER_LAUNCH], out[ROTATE_FRAMES_PER_LAUNCH];
    double a[ROTATE_FRAMES_PER_LAUNCH], b[ROTATE_FRAMES_PER_LAUNCH], cx[ROTATE_FRAMES_PER_LAUNCH], cy[ROTATE_FRAMES_PER_LAUNCH];
};

struct RotateParams {
    int W, H;
    StagePlan planW, planH;
    const float2 *twW, *twH;        // n-th roots exp(+2 pi i k / n)
    float2 *rg1, *rg2;              // [frame][H][W]: R + i G of the two intermediates
    float *b1, *b2;                 // [frame][H][W]: B
};

// one pixel of a caller's frame, the three channels (RGB8: code / 255)
__device__ __forceinline__ void rotate_load_px(const RotateImage& im, long x, long y, float* v)
{
    if (im.kind == 0) {
        const uint8_t* p = im.data + y * im.row + 3 * x;
        v[0] = (float)p[0] * (1.0f / 255.0f); v[1] = (float)p[1] * (1.0f / 255.0f); v[2] = (float)p[2] * (1.0f / 255.0f);
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint8_t* p = im.data + c * im.plane + y * im.row;
        if (im.kind == 1) v[c] = ((const float*)p)[x];
        else if (im.kind == 2) v[c] = __half2float(((const __half*)p)[x]);
        else if (im.kind == 3) {
            const uint8_t* q = p + 4 * x;
            v[c] = __uint_as_float((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24));
        } else {
            const uint8_t* q = p + 2 * x;
            v[c] = __half2float(__ushort_as_half((unsigned short)(q[0] | (q[1] << 8))));
        }
    }
}

__device__ __forceinline__ uint8_t rotate_u8(float x)
{
    const float t = floorf(fmaf(255.0f, x, 0.5f));
    return (uint8_t)fminf(fmaxf(t, 0.0f), 255.0f);       // (a NaN becomes 0)
}

// ... and one pixel into a caller's frame: exactly its own bytes
__device__ __forceinline__ void rotate_store_px(const RotateImage& im, long x, long y, const float* v)
{
    uint8_t* base = im.data;
    if (im.kind == 0) {
        uint8_t* p = base + y * im.row + 3 * x;
        p[0] = rotate_u8(v[0]); p[1] = rotate_u8(v[1]); p[2] = rotate_u8(v[2]);
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        uint8_t* p = base + c * im.plane + y * im.row;
        if (im.kind == 1) ((float*)p)[x] = v[c];
        else if (im.kind == 2) ((__half*)p)[x] = __float2half(v[c]);
        else if (im.kind == 3) {
            const uint32_t u = __float_as_uint(v[c]);
            uint8_t* q = p + 4 * x;
            q[0] = (uint8_t)u; q[1] = (uint8_t)(u >> 8); q[2] = (uint8_t)(u >> 16); q[3] = (uint8_t)(u >> 24);
        } else {
            const unsigned short u = __half_as_ushort(__float2half(v[c]));
            uint8_t* q = p + 2 * x;
            q[0] = (uint8_t)u; q[1] = (uint8_t)(u >> 8);
        }
    }
}

__device__ __forceinline__ float2 rotate_factor(int k, int n, double delta)
{
    const fftup_rotphase::Cplx w = fftup_rotphase::shear_factor(k, n, delta);
    return make_float2((float)w.re, (float)w.im);
}

// fftup_rotate_frames_angles: the shear coefficients of a chunk's frames from angles in device memory.  Frame i < n turns by
// theta = host.angle[i] + gain * (double)angles[i].angle (a device angle that is not finite counts as 0), clamped to [-pi/2, pi/2];
// coef[i] = (a, b) = (-tan(theta / 2), sin(theta)), what fftup_rotphase::shear_a / shear_b give the host path.  One workgroup.
constexpr int ROTATE_MAX_BATCH = 64;             // rotate_geometry's limit on max_batch: a chunk's host angles travel as an argument
struct RotateHostAngles { double angle[ROTATE_MAX_BATCH]; };
static __global__ void k_rotate_coeffs(RotateHostAngles host, const float* angles, double gain, int n, double2* coef)
{
    const int i = threadIdx.x;
    if (i >= n) return;
    const float m = angles[4 * (long)i];         // fftup_roll_angle: 4 floats, the angle first
    const double dm = isfinite(m) ? (double)m : 0.0;
    const double turn = gain * dm;
    double theta = host.angle[i] + turn;
    const double half_pi = 1.57079632679489661923;
    theta = fmin(fmax(theta, -half_pi), half_pi);
    coef[i] = make_double2(-tan(0.5 * theta), sin(theta));
}

// OUT = 0: the caller's frame q.in -> the first intermediate; OUT = 1: the second intermediate -> the caller's frame q.out.
// frame0: the launch's first frame within the chunk (the index of its intermediates); coef: the chunk's shear coefficients in
// device memory (k_rotate_coeffs), or null: q.a / q.b
template <int OUT>
static __global__ void k_rotate_shear_x(RotateParams p, RotateFrames q, int frame0, const double2* coef)
{
    extern __shared__ float2 rotate_lds[];
    const int y = blockIdx.x, fz = blockIdx.z, tid = threadIdx.x, T = blockDim.x, W = p.W;
    float2* a = rotate_lds;
    float2* b = a + lpad_size(2 * W);
    const long line = ((long)(frame0 + fz) * p.H + y) * W;
    if (OUT) {
        const float2* rg = p.rg2 + line;
        const float* bb = p.b2 + line;
        for (int x = tid; x < W; x += T) {
            a[lpad(2 * x)] = rg[x];
            a[lpad(2 * x + 1)] = make_float2(bb[x], 0.0f);
        }
    } else {
        const RotateImage& im = q.in[fz];
        for (int x = tid; x < W; x += T) {
            float v[3];
            rotate_load_px(im, x, y, v);
            a[lpad(2 * x)] = make_float2(v[0], v[1]);
            a[lpad(2 * x + 1)] = make_float2(v[2], 0.0f);
        }
    }
    __syncthreads();
    float2* f = fft_lds<-1, 2>(a, b, p.planW, p.twW, tid, T);
    float2* o = f == a ? b : a;
    const double sa = coef ? coef[frame0 + fz].x : q.a[fz];
    const double delta = sa * ((double)y - q.cy[fz]);
    for (int k = tid; k < W; k += T) {
        const float2 w = rotate_factor(k, W, delta);
        f[lpad(2 * k)] = cmul(f[lpad(2 * k)], w);
        f[lpad(2 * k + 1)] = cmul(f[lpad(2 * k + 1)], w);
    }
    __syncthreads();
    const float2* r = fft_lds<1, 2>(f, o, p.planW, p.twW, tid, T);
    const float s = 1.0f / (float)W;
    if (OUT) {
        const RotateImage& im = q.out[fz];
        for (int x = tid; x < W; x += T) {
            const float2 z = r[lpad(2 * x)];
            const float v[3] = {z.x * s, z.y * s, r[lpad(2 * x + 1)].x * s};
            rotate_store_px(im, x, y, v);
        }
    } else {
        float2* rg = p.rg1 + line;
        float* bb = p.b1 + line;
        for (int x = tid; x < W; x += T) {
            const float2 z = r[lpad(2 * x)];
            rg[x] = make_float2(z.x * s, z.y * s);
            bb[x] = r[lpad(2 * x + 1)].x * s;
        }
    }
}

// blockIdx.x: the tile of columns [TK blockIdx.x, TK blockIdx.x + TK) -- those at or beyond W are zeros in LDS and are never
// stored; blockIdx.y: 0 the sequence R + i G, 1 the sequence B + i 0; blockIdx.z: the frame of the chunk
template <int TK>
static __global__ void k_rotate_shear_y(RotateParams p, RotateFrames q, int frame0, const double2* coef)
{
    extern __shared__ float2 rotate_lds[];
    const int fz = blockIdx.z, tid = threadIdx.x, T = blockDim.x, W = p.W, H = p.H;
    const int x0 = blockIdx.x * TK;
    const bool seq_b = blockIdx.y != 0;
    float2* a = rotate_lds;
    float2* b = a + lpad_size(TK * H);
    const long frame = (long)(frame0 + fz) * H * W;
    for (int g = tid; g < TK * H; g += T) {
        const int x = x0 + g % TK, y = g / TK;
        float2 z = make_float2(0.0f, 0.0f);
        if (x < W) {
            const long at = frame + (long)y * W + x;
            if (seq_b) z.x = p.b1[at];
            else z = p.rg1[at];
        }
        a[lpad(g)] = z;
    }
    __syncthreads();
    float2* f = fft_lds<-1, TK>(a, b, p.planH, p.twH, tid, T);
    float2* o = f == a ? b : a;
    const double sb = coef ? coef[frame0 + fz].y : q.b[fz], cx = q.cx[fz];
    for (int g = tid; g < TK * H; g += T) {
        const double delta = sb * ((double)(x0 + g % TK) - cx);
        f[lpad(g)] = cmul(f[lpad(g)], rotate_factor(g / TK, H, delta));
    }
    __syncthreads();
    const float2* r = fft_lds<1, TK>(f, o, p.planH, p.twH, tid, T);
    const float s = 1.0f / (float)H;
    for (int g = tid; g < TK * H; g += T) {
        const int x = x0 + g % TK, y = g / TK;
        if (x >= W) continue;
        const long at = frame + (long)y * W + x;
        const float2 z = r[lpad(g)];
        if (seq_b) p.b2[at] = z.x * s;
        else p.rg2[at] = make_float2(z.x * s, z.y * s);
    }
}

}  // namespace fftup
