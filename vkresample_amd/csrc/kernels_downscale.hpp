// kernels_downscale.hpp -- size-generic HIP kernels of the FFT downscale mode (FFTUP_FLAG_DOWNSCALE, include/fftup.h): the spectrum
// is CROPPED to the output size instead of zero-padded.  Per axis, input length N, output length M < N (both even), h = M/2,
// X = DFT(x):  Y[k] = X[k] (k < h),  Y[h] = X[h] + X[N-h] (the two Nyquist bins folded),  Y[M-k] = X[N-k] (0 < k < h),  then
// (1/M) IDFT_M(Y).  Four launches per frame:
//   k_row_r2c_crop   R2C of the rows (pairs of rows), bins kx <= uW/2 only        input -> S1 blocked half spectrum, NTc tiles, H rows
//   k_col_crop       forward length H, fold + gather to uH rows, inverse length uH  S1 -> S2 (NTc tiles, uH rows), scaled by 1/uH
//   k_row_c2r        the upscale path's C2R (kernels_generic.hpp) with W := uW and an empty read guard, scaled by 1/uW
//   k_sharpen        the upscale path's sharpen pass, unchanged
// NTc = ceil((uW/2 + 1) / TK): the row stage already drops the bins the output cannot hold, so S1 and the column work shrink with
// the output width.  For a real row the folded Nyquist bin X[h] + X[W-h] = 2 Re X[h] is real: it is stored as (2 Re A, 0) and
// (2 Re B, 0) for the row pair, and the C2R kernel's two writes of a[uW/2] (k = uW/2 and uW - k) then agree.  fp32 arithmetic;
// -p 2 stores R as binary16 (k_row_c2r<true>).
// FFTUP_FLAG_ANY_SIZE: the BZ instantiations run each transform whose length is not smooth as a Bluestein transform
// (kernels_bluestein.hpp, chosen per transform by the BzPlan members of the parameters); their LDS buffers are sized by L * TK.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "fft_engine.hpp"
#include "kernels_bluestein.hpp"
#include "kernels_generic.hpp"

namespace fftup {

struct DownRowParams {
    const void* in;          // planar float/half (row stride, plane stride in elements) or u8 RGB (row stride bytes)
    float2* S1;              // blocked half spectrum, H rows, NT tiles of TK columns
    const float2* tw;        // W-th roots
    StagePlan plan;          // n = W
    int W, H;
    long in_row_stride, in_plane_stride;
    int TK, NT;              // tile width (complex), number of tiles = ceil((h + 1) / TK)
    int h;                   // uW / 2: the last bin kept (folded)
    BzPlan bz;               // BZ instantiations: the rows' Bluestein transform
};

// grid (H/2, 3); dynamic LDS = 2 * lpad_size(W) complex (BZ: of bz.L).  Rows 2j (real part) and 2j+1 (imaginary part).
template <int MODE, bool BZ = false>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_row_r2c_crop(DownRowParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(BZ ? p.bz.L : p.W);
    const int tid = threadIdx.x, T = blockDim.x;
    const int j = blockIdx.x, c = blockIdx.y;
    const int W = p.W, h = p.h;
    for (int n = tid; n < W; n += T)
        a[lpad(n)] = make_float2((float)load_px<MODE>(p, c, 2 * j, n), (float)load_px<MODE>(p, c, 2 * j + 1, n));
    __syncthreads();
    const float2* Z;
    if constexpr (BZ) Z = fft_bluestein<+1, 1>(a, b, W, p.bz, tid, T);
    else Z = fft_lds<+1, 1>(a, b, p.plan, p.tw, tid, T);
    // unpack as k_row_r2c: A = (Z[k] + conj Z[W-k]) / 2, B = (Z[k] - conj Z[W-k]) / 2i; at k = h: 2 Re A, 2 Re B (h < W/2)
    const long tile_stride = (long)p.H * p.TK;
    float2* base = p.S1 + (long)c * p.NT * tile_stride;
    for (int k = tid; k <= h; k += T) {
        const float2 zk = Z[lpad(k)];
        const float2 zn = Z[lpad(k == 0 ? 0 : W - k)];
        float2 A, B;
        if (k < h) {
            A = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
            B = make_float2(0.5f * (zk.y + zn.y), 0.5f * (-zk.x + zn.x));
        } else {
            A = make_float2(zk.x + zn.x, 0.f);
            B = make_float2(zk.y + zn.y, 0.f);
        }
        float2* dst = base + (long)(k / p.TK) * tile_stride + (long)(2 * j) * p.TK + (k % p.TK);
        dst[0] = A;
        dst[p.TK] = B;
    }
}

struct DownColParams {
    const float2* S1;        // H rows per tile
    float2* S2;              // uH rows per tile
    const float2 *twH, *twUH;
    StagePlan planH, planUH;
    int H, uH;
    int NT;
    int ncols;               // kx columns present: uW/2 + 1
    float inv_norm;          // 1/uH
    BzPlan bzH, bzUH;        // BZ instantiations: per transform, L = 0 for a smooth length
};

// grid (NT, 3); dynamic LDS = 2 * lpad_size(H*TK) complex (the forward transform is the longer one; BZ: max(H, bzH.L, bzUH.L) * TK)
template <int TK, bool BZ = false>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_col_crop(DownColParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size((BZ ? max(p.H, max(p.bzH.L, p.bzUH.L)) : p.H) * TK);
    const int tid = threadIdx.x, T = blockDim.x;
    const int tile = blockIdx.x, c = blockIdx.y;
    const int H = p.H, uH = p.uH, hh = p.uH / 2;
    const int ncol_valid = min(TK, p.ncols - tile * TK);
    load_col_tile<TK>(a, p.S1 + ((long)c * p.NT + tile) * H * TK, H, ncol_valid, tid, T);
    __syncthreads();
    float2* F;
    if constexpr (BZ) F = fft_any<+1, TK>(a, b, p.planH, p.twH, p.bzH, tid, T);
    else F = fft_lds<+1, TK>(a, b, p.planH, p.twH, tid, T);
    float2* G = (F == a) ? b : a;
    // crop: rows below hh as they are, row hh = F[hh] + F[H - hh], rows above hh from uH - H rows further on
    for (int e = tid; e < uH * TK; e += T) {
        const int ky = e / TK, col = e % TK;
        float2 v;
        if (ky < hh) v = F[lpad(e)];
        else if (ky == hh) v = cadd(F[lpad(e)], F[lpad((H - hh) * TK + col)]);
        else v = F[lpad(e + (H - uH) * TK)];
        G[lpad(e)] = v;
    }
    __syncthreads();
    const float2* D;
    if constexpr (BZ) D = fft_any<-1, TK>(G, F, p.planUH, p.twUH, p.bzUH, tid, T);
    else D = fft_lds<-1, TK>(G, F, p.planUH, p.twUH, tid, T);
    store_col_tile<TK>(p.S2 + ((long)c * p.NT + tile) * uH * TK, D, uH, ncol_valid, p.inv_norm, tid, T);
}

}  // namespace fftup
