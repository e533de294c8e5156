// kernels_align.hpp -- shift estimates (include/fftup.h, fftup_align_shifts): band-limited phase-only correlation of frame pairs
// with a sub-pixel refinement.  Five kernels per chunk of pairs, the pair in blockIdx.z, nothing read by the host in between:
//   k_align_rows       one workgroup per window row: luma, d x d box mean, crop and window of BOTH frames, z = a + i b in LDS,
//                      forward row transform (fft_lds, radices 8/4/2), Z rows to HBM; the row's DC bin also to `dc`
//   k_align_cols       one workgroup per column PAIR (k_x, n_x - k_x) of the band: both columns side by side in LDS (TK = 2),
//                      forward column transforms, A / B separated from Z[k] and conj Z[-k] -- the partner bin lives in the OTHER column
//                      of the pair, which is why a pair shares a workgroup -- R = P / |P| with the band and floor rules, R to the band
//                      buffer the fine stage reads, inverse column transforms, result back into the pair's own two columns of Z
//   k_align_peak_rows  one workgroup per row: inverse row transform (columns outside the band are zeros, never read), the row's
//                      maximum with the lowest x on a tie (wave shuffles, then the waves' results through LDS)
//   k_align_fine_x     one workgroup per k_y row of the band: the coarse peak from the rows' maxima, then the first product of the
//                      separable interpolant, G[k_y][i] = sum_kx R[k_y][k_x] exp(2 pi i k_x (p_x + i / kappa) / n_x)
//   k_align_fine_y     one workgroup per pair: r(u_i, v_j) = Re sum_ky G[k_y][i] exp(2 pi i k_y (p_y + j / kappa) / n_y), argmax,
//                      the parabola per axis, one 16-byte store of the fftup_shift
// Phases of the fine stage are exact: k (p kappa + i) is reduced modulo kappa n in integers and looked up in a table of the
// (kappa n)-th roots computed in double.  Transform direction: fft_engine's DIR = -1 is numpy's forward DFT.
// LDS: rows 2 lpad(n_x) float2 (17.4 KB at 1024); columns 2 lpad(2 n_y) float2 (34.8 KB at 1024: two buffers x 2 columns x 1024
// float2 and the padding); the fine kernels 8 KB and below.  Not handed to the plan-time compiler.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_engine.hpp"

namespace fftup {

// one frame: kind 0 RGB8, 1 float planes, 2 half planes, 3 / 4 the same planes at an address that is no multiple of the element
// size (assembled from bytes); strides in bytes
struct AlignImage { const uint8_t* data; long row, plane; int kind; };
constexpr int ALIGN_PAIRS_PER_LAUNCH = 16;       // descriptors travel as kernel arguments: read before the launch returns
struct AlignPairs { AlignImage ref[ALIGN_PAIRS_PER_LAUNCH], cur[ALIGN_PAIRS_PER_LAUNCH]; };

struct AlignParams {
    int nx, ny, d, crop_x, crop_y, kappa, bkx, bky, Kx, Ky;
    StagePlan planX, planY;
    const float2 *twX, *twY;        // n-th roots exp(+2 pi i k / n)
    const float *winX, *winY;       // w[n] = 1/2 - 1/2 cos(2 pi (n + 1/2) / N)
    const float2 *phX, *phY;        // (kappa n)-th roots
    float2* Z;                      // [pair][n_y][n_x]: Z rows, then the column pass' result in the band's columns
    float2* dc;                     // [pair][n_y]: bin k_x = 0 of every Z row (their sum is Z[0,0])
    float2* Rb;                     // [pair][Ky][Kx]: R in the band, index k + band_k per axis
    float2* Gx;                     // [pair][Ky][2 kappa + 1]
    float2* part;                   // [pair][n_y]: (row maximum, its x as int bits)
};

__device__ __forceinline__ float align_luma(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

__device__ __forceinline__ float align_px(const AlignImage& im, long x, long y)
{
    if (im.kind == 0) {
        const uint8_t* p = im.data + y * im.row + 3 * x;
        return align_luma((float)p[0], (float)p[1], (float)p[2]) * (1.0f / 255.0f);
    }
    float v[3];
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
    return align_luma(v[0], v[1], v[2]);
}

// step 1 of the estimate for window pixel (x, y) of a pair: the d x d sums of both frames' luma times w, the product of the window
// and 1 / d^2 -- (a, b) of z = a + i b.  Shared with the roll estimator (kernels_roll.hpp)
__device__ __forceinline__ float2 align_window_px(const AlignImage& R, const AlignImage& C, int crop_x, int crop_y, int d, int x, int y, float w)
{
    float sa = 0.0f, sb = 0.0f;
    for (int j = 0; j < d; j++)
        for (int i = 0; i < d; i++) {
            const long X = crop_x + (long)x * d + i, Y = crop_y + (long)y * d + j;
            sa += align_px(R, X, Y);
            sb += align_px(C, X, Y);
        }
    return make_float2(sa * w, sb * w);
}

// the better of two candidates: the larger value, the lower index on a tie
__device__ __forceinline__ void align_better(float& v, int& i, float ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// argmax over the workgroup (T a multiple of 64, at most 1024): every thread returns with the winner; sv / si: 16 entries of LDS
__device__ __forceinline__ void align_block_argmax(float& v, int& i, float* sv, int* si, int tid, int T)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const float ov = __shfl_down(v, off);
        const int oi = __shfl_down(i, off);
        align_better(v, i, ov, oi);
    }
    __syncthreads();                                  // (sv / si may still be read from an earlier call)
    if ((tid & 63) == 0) { sv[tid >> 6] = v; si[tid >> 6] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
    for (int w = 1; w < (T >> 6); w++) align_better(v, i, sv[w], si[w]);
}

static __global__ void k_align_rows(AlignParams p, AlignPairs q, int pair0)
{
    extern __shared__ float2 align_lds[];
    const int y = blockIdx.x, pz = blockIdx.z, tid = threadIdx.x, T = blockDim.x, nx = p.nx, d = p.d;
    float2* a = align_lds;
    float2* b = a + lpad_size(nx);
    const AlignImage& R = q.ref[pz];
    const AlignImage& C = q.cur[pz];
    const float wy = p.winY[y] / (float)(d * d);
    for (int x = tid; x < nx; x += T) a[lpad(x)] = align_window_px(R, C, p.crop_x, p.crop_y, d, x, y, p.winX[x] * wy);
    __syncthreads();
    const float2* r = fft_lds<-1, 1>(a, b, p.planX, p.twX, tid, T);
    const long row = (long)(pair0 + pz) * p.ny + y;
    float2* Z = p.Z + row * nx;
    for (int x = tid; x < nx; x += T) Z[x] = r[lpad(x)];
    if (tid == 0) p.dc[row] = r[lpad(0)];
}

static __global__ void k_align_cols(AlignParams p)
{
    extern __shared__ float2 align_lds[];
    const int tid = threadIdx.x, T = blockDim.x, nx = p.nx, ny = p.ny, pz = blockIdx.z;
    const int c0 = blockIdx.x, c1 = (nx - c0) % nx;
    const bool same = c0 == c1;                       // k_x = 0 and k_x = n_x / 2 are their own partners: both halves hold the column
    float2* a = align_lds;
    float2* b = a + lpad_size(2 * ny);
    float2* red = b + lpad_size(2 * ny);              // T entries
    float2* Z = p.Z + (long)pz * ny * nx;
    for (int g = tid; g < 2 * ny; g += T) a[lpad(g)] = Z[(long)(g >> 1) * nx + ((g & 1) ? c1 : c0)];
    // Z[0,0] = A[0,0] + i B[0,0]: the sum of the rows' DC bins, in one fixed order for every workgroup of the pair
    float2 s = make_float2(0.0f, 0.0f);
    for (int y = tid; y < ny; y += T) { const float2 v = p.dc[(long)pz * ny + y]; s.x += v.x; s.y += v.y; }
    red[tid] = s;
    __syncthreads();
    for (int h = T >> 1; h; h >>= 1) {
        if (tid < h) { red[tid].x += red[tid + h].x; red[tid].y += red[tid + h].y; }
        __syncthreads();
    }
    // P[0,0] = 0: a frame that is black in the window.  Its transform is zero in exact arithmetic, but A and B come out of ONE packed
    // transform, and the separation leaves a rounding residue of the other frame in it -- unit phasors of noise that a floor of 0
    // would let through (a peak of 0.14 at 64 x 32).  Such a pair has no signal: R = 0 everywhere.
    const float p00 = fabsf(red[0].x * red[0].y);
    const bool live = p00 > 0.0f;
    const float floor_p = 1e-9f * p00;
    float2* f = fft_lds<-1, 2>(a, b, p.planY, p.twY, tid, T);
    float2* o = f == a ? b : a;
    const int sx0 = c0 < nx - c0 ? c0 : c0 - nx;      // signed k_x of the two columns, in [-n_x/2, n_x/2)
    const int sx1 = c1 < nx - c1 ? c1 : c1 - nx;
    for (int g = tid; g < 2 * ny; g += T) {
        const int col = g & 1, ky = g >> 1, kym = (ny - ky) % ny;
        const float2 zk = f[lpad(g)], zm = f[lpad(2 * kym + (1 - col))];
        const float2 A = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
        const float2 B = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
        const float2 P = make_float2(B.x * A.x + B.y * A.y, B.y * A.x - B.x * A.y);
        const float mag = hypotf(P.x, P.y);
        const int sy = ky < ny - ky ? ky : ky - ny;
        const bool band = (sy < 0 ? -sy : sy) <= p.bky;
        float2 Rv = make_float2(0.0f, 0.0f);
        if (band && live && mag > floor_p) Rv = make_float2(P.x / mag, P.y / mag);
        o[lpad(g)] = Rv;
        if (band && !(same && col)) p.Rb[((long)pz * p.Ky + (sy + p.bky)) * p.Kx + ((col ? sx1 : sx0) + p.bkx)] = Rv;
    }
    __syncthreads();
    const float2* r = fft_lds<1, 2>(o, f, p.planY, p.twY, tid, T);
    for (int g = tid; g < 2 * ny; g += T)
        if (!(same && (g & 1))) Z[(long)(g >> 1) * nx + ((g & 1) ? c1 : c0)] = r[lpad(g)];
}

static __global__ void k_align_peak_rows(AlignParams p)
{
    extern __shared__ float2 align_lds[];
    __shared__ float sv[16];
    __shared__ int si[16];
    const int y = blockIdx.x, pz = blockIdx.z, tid = threadIdx.x, T = blockDim.x, nx = p.nx;
    float2* a = align_lds;
    float2* b = a + lpad_size(nx);
    const long row = (long)pz * p.ny + y;
    const float2* Z = p.Z + row * nx;
    const int bc = p.bkx < nx / 2 ? p.bkx : nx / 2;   // the column pass wrote columns [0, bc] and [n_x - bc, n_x)
    for (int x = tid; x < nx; x += T) a[lpad(x)] = (x <= bc || x >= nx - bc) ? Z[x] : make_float2(0.0f, 0.0f);
    __syncthreads();
    const float2* r = fft_lds<1, 1>(a, b, p.planX, p.twX, tid, T);
    float v = -INFINITY;
    int i = 0x7fffffff;
    for (int x = tid; x < nx; x += T) align_better(v, i, r[lpad(x)].x, x);
    align_block_argmax(v, i, sv, si, tid, T);
    if (tid == 0) p.part[row] = make_float2(v, __int_as_float(i));
}

// the coarse peak of a pair from its rows' maxima: value (unscaled: n_x n_y r) and the row-major index y n_x + x
__device__ __forceinline__ void align_coarse_peak(const AlignParams& p, int pz, float& v, int& idx, float* sv, int* si, int tid, int T)
{
    v = -INFINITY;
    idx = 0x7fffffff;
    for (int y = tid; y < p.ny; y += T) {
        const float2 m = p.part[(long)pz * p.ny + y];
        align_better(v, idx, m.x, y * p.nx + __float_as_int(m.y));
    }
    align_block_argmax(v, idx, sv, si, tid, T);
}

// index of exp(2 pi i k (pk + i) / (kappa n)) in the table of M = kappa n roots, for the first k of a run; q: the step per k
__device__ __forceinline__ uint32_t align_phase_start(int k, int pk_plus_i, uint32_t M, uint32_t* q)
{
    int qq = pk_plus_i % (int)M;
    if (qq < 0) qq += (int)M;
    int kk = k % (int)M;
    if (kk < 0) kk += (int)M;
    *q = (uint32_t)qq;
    return (uint32_t)(((uint64_t)kk * (uint64_t)qq) % M);
}

static __global__ void k_align_fine_x(AlignParams p)
{
    __shared__ float2 row[1024];
    __shared__ float sv[16];
    __shared__ int si[16];
    const int iy = blockIdx.x, pz = blockIdx.z, tid = threadIdx.x, T = blockDim.x, Kx = p.Kx, nf = 2 * p.kappa + 1;
    float v;
    int idx;
    align_coarse_peak(p, pz, v, idx, sv, si, tid, T);
    const int px = idx % p.nx;
    const float2* Rrow = p.Rb + ((long)pz * p.Ky + iy) * Kx;
    for (int k = tid; k < Kx; k += T) row[k] = Rrow[k];
    __syncthreads();
    const uint32_t M = (uint32_t)(p.kappa * p.nx);
    for (int i = tid; i < nf; i += T) {
        uint32_t q;
        uint32_t m = align_phase_start(-p.bkx, px * p.kappa + i - p.kappa, M, &q);
        double ax = 0.0, ay = 0.0;                    // (fp64 sums: up to 1024 terms, and the vector fp64 rate is the fp32 rate here)
        for (int k = 0; k < Kx; k++) {
            const float2 e = p.phX[m], rr = row[k];
            ax += (double)rr.x * (double)e.x - (double)rr.y * (double)e.y;
            ay += (double)rr.x * (double)e.y + (double)rr.y * (double)e.x;
            m += q;
            if (m >= M) m -= M;
        }
        p.Gx[((long)pz * p.Ky + iy) * nf + i] = make_float2((float)ax, (float)ay);
    }
}

// n_x n_y r(p_x + (i - kappa) / kappa, p_y + (j - kappa) / kappa): the second product, over k_y
__device__ __forceinline__ float align_fine_value(const AlignParams& p, const float2* G, int py, int i, int j)
{
    const int nf = 2 * p.kappa + 1;
    const uint32_t M = (uint32_t)(p.kappa * p.ny);
    uint32_t q;
    uint32_t m = align_phase_start(-p.bky, py * p.kappa + j - p.kappa, M, &q);
    double acc = 0.0;
    for (int k = 0; k < p.Ky; k++) {
        const float2 e = p.phY[m], g = G[(long)k * nf + i];
        acc += (double)g.x * (double)e.x - (double)g.y * (double)e.y;
        m += q;
        if (m >= M) m -= M;
    }
    return (float)acc;
}

static __global__ void k_align_fine_y(AlignParams p, float* shifts)
{
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ float nb[4];
    const int pz = blockIdx.z, tid = threadIdx.x, T = blockDim.x, kappa = p.kappa, nf = 2 * kappa + 1;
    float vc;
    int idx;
    align_coarse_peak(p, pz, vc, idx, sv, si, tid, T);
    const int px = idx % p.nx, py = idx / p.nx;
    const float2* G = p.Gx + (long)pz * p.Ky * nf;
    float v = -INFINITY;
    int best = 0x7fffffff;
    for (int t = tid; t < nf * nf; t += T) align_better(v, best, align_fine_value(p, G, py, t % nf, t / nf), t);
    align_block_argmax(v, best, sv, si, tid, T);
    const int bi = best % nf, bj = best / nf;
    // the fine neighbours of the maximum: x - 1, x + 1, y - 1, y + 1 (recomputed: the same sums, the same bits)
    if (tid < 4) {
        const int ni = bi + (tid == 0 ? -1 : tid == 1 ? 1 : 0), nj = bj + (tid == 2 ? -1 : tid == 3 ? 1 : 0);
        nb[tid] = (ni >= 0 && ni < nf && nj >= 0 && nj < nf) ? align_fine_value(p, G, py, ni, nj) : 0.0f;
    }
    __syncthreads();
    if (tid == 0) {
        float dx = 0.0f, dy = 0.0f;
        if (bi > 0 && bi < nf - 1) {
            const float den = nb[0] - 2.0f * v + nb[1];
            if (den != 0.0f) dx = 0.5f * (nb[0] - nb[1]) / den;
        }
        if (bj > 0 && bj < nf - 1) {
            const float den = nb[2] - 2.0f * v + nb[3];
            if (den != 0.0f) dy = 0.5f * (nb[2] - nb[3]) / den;
        }
        float sx = (float)px + ((float)(bi - kappa) + dx) / (float)kappa;
        float sy = (float)py + ((float)(bj - kappa) + dy) / (float)kappa;
        sx -= (float)p.nx * floorf((sx + 0.5f * (float)p.nx) / (float)p.nx);
        sy -= (float)p.ny * floorf((sy + 0.5f * (float)p.ny) / (float)p.ny);
        const float K = (float)p.Kx * (float)p.Ky;
        const float4 res = make_float4((float)p.d * sx, (float)p.d * sy, v / K, vc / K);
        float* out = shifts + 4 * (long)pz;
        if (((uintptr_t)out & 15) == 0) *(float4*)out = res;
        else { out[0] = res.x; out[1] = res.y; out[2] = res.z; out[3] = res.w; }
    }
}

}  // namespace fftup
