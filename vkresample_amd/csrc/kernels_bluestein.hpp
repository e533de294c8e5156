// kernels_bluestein.hpp -- FFTUP_FLAG_ANY_SIZE (include/fftup.h): transforms of lengths with a prime factor above 7.
//
// fft_bluestein has the calling shape of fft_lds (fft_engine.hpp): TK interleaved sequences in LDS as complex [n][TK], two
// buffers, returns the buffer that holds the result.  It computes the length-N DFT X[k] = sum_n x[n] exp(DIR 2 pi i nk / N) for
// ANY N as a chirp-z transform: with nk = (n^2 + k^2 - (k - n)^2) / 2 and w[n] = exp(DIR i pi n^2 / N),
//     X[k] = w[k] * sum_n (x[n] w[n]) conj(w)[k - n]
// -- a convolution, run as a cyclic one of a smooth length L >= 2N - 1 through the Stockham stages that exist:
//     a[n] = x[n] w[n] (zero up to L),  A = FFT_L(a),  A[k] *= Bhat[k],  c = IFFT_L(A),  X[k] = c[k] w[k]
// with Bhat = FFT_L(conj w, wrapped) / L.  conj w is even in n, so the table of the other direction is the conjugate: both
// tables are stored for DIR = +1 and conjugated on the way in (twid<DIR>).  They come from the host, evaluated in double with the
// phase reduced as (n^2 mod 2N) in 64-bit integers and rounded once to fp32 (fftup_plan.hip: pi n^2 / N reaches thousands of
// radians -- formed in fp32 it is off by ~1e-3 rad at N of a few thousand; tests/test_host_anysize.py keeps the comparison), and
// are read from global memory (at most 64 KB per length: L2 resident).
//
// The kernels below are the size-generic column and row C2R kernels of kernels_generic.hpp -- same parameters, same spectrum
// layout, same unpacking / shift / read-guard code around the transforms -- with every transform chosen PER TRANSFORM: Bluestein
// where its BzPlan says so (L != 0), fft_lds where the length is smooth.  Buffers are sized by L * TK.  (Bluestein rows of the
// forward pass run k_row_r2c_odd, kernels_odd.hpp: its unpack is the size-generic one.)
// They live here and not behind a template flag in kernels_generic.hpp because that file is part of the sources the plan-time
// compiler embeds and the committed counter profiles are fingerprinted on (bench.py kernel_sources_sha256): plans that are valid
// without the flag keep their kernels, binaries and fingerprints byte for byte.  fp32 arithmetic only (no -p 1 Bluestein plans).
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "bluestein_plan.hpp"
#include "fft_engine.hpp"
#include "kernels_generic.hpp"

namespace fftup {

// Data in `a`, N * TK points (valid after a barrier executed by the caller); both buffers hold lpad_size(z.L * TK) points;
// returns the buffer holding the N * TK results (synced).
template <int DIR, int TK>
__device__ __forceinline__ float2* fft_bluestein(float2* a, float2* b, int N, const BzPlan& z, int tid, int T)
{
    const int L = z.L;
    for (int e = tid; e < L * TK; e += T) {
        const int n = e / TK;
        float2 v = make_float2(0.f, 0.f);
        if (n < N) v = cmul(a[lpad(e)], twid<DIR>(z.chirp[n]));
        a[lpad(e)] = v;
    }
    __syncthreads();
    float2* A = fft_lds<+1, TK>(a, b, z.plan, z.tw, tid, T);
    float2* B = (A == a) ? b : a;
    for (int e = tid; e < L * TK; e += T) A[lpad(e)] = cmul(A[lpad(e)], twid<DIR>(z.bhat[e / TK]));
    __syncthreads();
    float2* c = fft_lds<-1, TK>(A, B, z.plan, z.tw, tid, T);
    for (int e = tid; e < N * TK; e += T) c[lpad(e)] = cmul(c[lpad(e)], twid<DIR>(z.chirp[e / TK]));
    __syncthreads();
    return c;
}

// one transform of a plan: Bluestein or direct (wave-uniform choice)
template <int DIR, int TK>
__device__ __forceinline__ float2* fft_any(float2* a, float2* b, const StagePlan& P, const float2* __restrict__ tw, const BzPlan& z, int tid, int T)
{
    if (z.L) return fft_bluestein<DIR, TK>(a, b, P.n, z, tid, T);
    return fft_lds<DIR, TK>(a, b, P, tw, tid, T);
}

// ---- what the column and inverse row kernels here, in kernels_downscale.hpp, kernels_odd.hpp and kernels_view.hpp share
// one tile of a blocked half spectrum, `rows` rows of TK columns at `src`, into LDS; the columns the spectrum does not have as zeros
template <int TK>
__device__ __forceinline__ void load_col_tile(float2* a, const float2* src, int rows, int ncol_valid, int tid, int T)
{
    for (int e = tid; e < rows * TK; e += T) {
        float2 v = make_float2(0.f, 0.f);
        if ((e % TK) < ncol_valid) v = src[e];
        a[lpad(e)] = v;
    }
}
// ... and back: the columns that exist, as they are or times `s`
template <int TK>
__device__ __forceinline__ void store_col_tile(float2* dst, const float2* D, int rows, int ncol_valid, int tid, int T)
{
    for (int e = tid; e < rows * TK; e += T)
        if ((e % TK) < ncol_valid) dst[e] = D[lpad(e)];
}
template <int TK>
__device__ __forceinline__ void store_col_tile(float2* dst, const float2* D, int rows, int ncol_valid, float s, int tid, int T)
{
    for (int e = tid; e < rows * TK; e += T)
        if ((e % TK) < ncol_valid) dst[e] = cscale(D[lpad(e)], s);
}
// element n of the row that starts at element `row` of the dense image R[3][uH][uW], fp32 or binary16.  (The inverse row kernels
// store one element at a time: with an odd uW the second row of a pair is not 4-byte aligned as binary16)
template <bool HALF_OUT>
__device__ __forceinline__ void store_px(void* R, long row, int n, float v)
{
    if constexpr (HALF_OUT) ((__half*)R + row)[n] = __float2half_rn(v);
    else ((float*)R + row)[n] = v;
}

// k_col (two-buffer form) with either transform Bluestein.  grid (NT, 3); dynamic LDS = 2 * lpad_size(nbuf * TK) complex,
// nbuf = max(uH, zH.L, zUH.L)
template <int TK>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_col_bz(ColParams p, BzPlan zH, BzPlan zUH)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(max(p.uH, max(zH.L, zUH.L)) * TK);
    const int tid = threadIdx.x, T = blockDim.x;
    const int tile = blockIdx.x, c = blockIdx.y;
    const int H = p.H, uH = p.uH;
    const int ncol_valid = min(TK, p.ncols - tile * TK);
    load_col_tile<TK>(a, p.S1 + ((long)c * p.NT + tile) * H * TK, H, ncol_valid, tid, T);
    __syncthreads();
    float2* F = fft_any<+1, TK>(a, b, p.planH, p.twH, zH, tid, T);
    float2* G = (F == a) ? b : a;
    // shift (VkResample.cpp:514-526) and the zero-padding read guard of the inverse plan, as k_col
    for (int e = tid; e < uH * TK; e += T) {
        const int ky = e / TK, col = e % TK;
        float2 v = make_float2(0.f, 0.f);
        if (!(ky >= p.zly && ky < p.zry)) {
            if (ky >= uH - H / 2) v = F[lpad((ky - (uH - H)) * TK + col)];
            else if (ky < H) v = F[lpad(e)];
        }
        G[lpad(e)] = v;
    }
    __syncthreads();
    const float2* D = fft_any<-1, TK>(G, F, p.planUH, p.twUH, zUH, tid, T);
    store_col_tile<TK>(p.S2 + ((long)c * p.NT + tile) * uH * TK, D, uH, ncol_valid, p.inv_norm, tid, T);
}

// k_row_c2r with a Bluestein transform of the rows.  grid (uH/2, 3); dynamic LDS = 2 * lpad_size(z.L) complex
template <bool HALF_OUT>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_row_c2r_bz(RowC2RParams p, BzPlan z)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(z.L);
    const int tid = threadIdx.x, T = blockDim.x;
    const int j = blockIdx.x, c = blockIdx.y;
    const int uW = p.uW;
    // rows 2j and 2j+1 of the spectrum after the column pass, as k_row_c2r (poly: even rows from S1, odd rows from S2)
    const long tile_stride = (long)(p.poly ? p.uH / 2 : p.uH) * p.TK;
    const float2* baseA = (p.poly ? p.S1 + (long)j * p.TK : p.S2 + (long)(2 * j) * p.TK) + (long)c * p.NT * tile_stride;
    const float2* baseB = (p.poly ? p.S2 + (long)j * p.TK : p.S2 + (long)(2 * j + 1) * p.TK) + (long)c * p.NT * tile_stride;
    const float sa = p.poly ? 0.5f : 1.0f;
    // vkFFT.h:2059-2131: Z[k] = A + iB, Z[uW-k] = conj(A) + i conj(B); column index cidx = k-1
    for (int cidx = tid; cidx < uW / 2; cidx += T) {
        const int k = cidx + 1;
        float2 A = make_float2(0.f, 0.f), B = A;
        if ((cidx < p.zlx || cidx >= p.zrx) && k <= p.W / 2) {
            const long o = (long)(k / p.TK) * tile_stride + (k % p.TK);
            A = cscale(baseA[o], sa);
            B = baseB[o];
        }
        a[lpad(k)] = make_float2(A.x - B.y, A.y + B.x);
        a[lpad(uW - k)] = make_float2(A.x + B.y, -A.y + B.x);
    }
    if (tid == 0) {
        const float2 A = cscale(baseA[0], sa), B = baseB[0];
        a[lpad(0)] = make_float2(A.x - B.y, A.y + B.x);
    }
    __syncthreads();
    const float2* zz = fft_bluestein<-1, 1>(a, b, uW, z, tid, T);
    const long plane = (long)uW * p.uH, row = c * plane + (long)(2 * j) * uW;
    for (int n = tid; n < uW; n += T) {
        const float2 v = cscale(zz[lpad(n)], p.inv_norm);
        store_px<HALF_OUT>(p.R, row, n, v.x);
        store_px<HALF_OUT>(p.R, row, uW + n, v.y);
    }
}

}  // namespace fftup
