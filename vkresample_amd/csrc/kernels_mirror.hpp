// kernels_mirror.hpp -- view plans with FFTUP_FLAG_MIRROR (include/fftup.h): the view of the frame's half-sample even reflection
// instead of its periodic continuation.
//
// Per axis, separable: x~[n] = x[n] (n < N), x~[n] = x[2N-1-n] (N <= n < 2N), period 2N.  Its spectrum is
//     X~[f] = 2 exp(i pi f / 2N) C[|f|],     C[k] = sum_n x[n] cos(pi k (2n+1) / 2N)  (DCT-II; C[N] = 0),
// so the view formula of kernels_view.hpp at period 2N and origin + 1/2 -- the tables of mirror_tables.hpp: pre[j] carries
// exp(i pi f (2 origin + 1) / 2N), g = 1/2 lands on the zero bin |f| = N, post carries 1/(2N) (span/M) -- takes
//     Z_f = 2 C[|f|],  |f| <= kmax,   0 where |f| = N.
// The factor 2 is applied here, where Z is gathered, and nowhere else.  fft_czt (kernels_view.hpp) runs unchanged.
//
// C comes from ONE transform of N points, not 2N: with v[q] = x[2q] (q < ceil(N/2)), v[N-1-q] = x[2q+1] (q < floor(N/2)),
// V = DFT_N(v), w_k = exp(-i pi k / 2N):
//     real x:     C[k] = Re(w_k V[k]),  C[N-k] = -Im(w_k V[k])          k = 0 .. N/2 (floor)
//     complex z:  2 C[k] = w_k V[k] + conj(w_k) V[(N-k) mod N]
// The forward transforms run with exp(+2 pi i nk / N) (fft_any<+1>), as in kernels_odd.hpp: bin k of the kernels holds the
// frequency -k, U[k] = V[-k] -- for a real row conj(V[k]).  With rot[k] = exp(+i pi k / 2N) = conj(w_k) (the DCT plans' table):
//     real rows:  C[k] = Re(rot[k] U[k]),  C[N-k] = Im(rot[k] U[k]);      columns:  2 C[k] = conj(rot[k]) F[(N-k) mod N] + rot[k] F[k].
// The column pass is a real matrix applied along y, so it maps the U-form half spectra of the input rows to the U-form half
// spectra of the output rows, and the inverse row kernel takes Re / Im of those.
//
// A frame is k_row_r2c_mirror (the reordered rows' unphased half spectra U[0 .. W/2]; only U[0 .. kmax_x] when kmax_x < W/2) ->
// k_col_view_mirror -> k_row_view_c2r_mirror -> the sharpen pass.  New parameter structs live here: kernels_generic.hpp,
// kernels_odd.hpp and kernels_view.hpp are fingerprinted by the committed counter profiles and stay byte-identical.  fp32
// arithmetic only (-p 0 and -p 2).
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "bluestein_plan.hpp"
#include "fft_engine.hpp"
#include "kernels_bluestein.hpp"
#include "kernels_generic.hpp"
#include "kernels_odd.hpp"
#include "kernels_view.hpp"

namespace fftup {

// where sample n of N goes before the transform: the even samples in order from the front, the odd ones in order from the back
__device__ __forceinline__ int mirror_slot(int n, int N) { return (n & 1) ? N - 1 - (n >> 1) : (n >> 1); }

struct MirrorRowParams {
    const void* in;          // planar float/half (row stride, plane stride in elements) or u8 RGB (row stride bytes)
    float2* S1;              // blocked half spectrum, H rows, ncols columns
    const float2* tw;        // W-th roots (direct transform)
    StagePlan plan;          // n = W
    int W, H;
    long in_row_stride, in_plane_stride;
    int TK, NT;              // tile width (complex), number of tiles = ceil(ncols / TK)
    int ncols;               // bins stored: kmax_x + 1 when kmax_x < W/2, else W/2 + 1
    BzPlan bz;               // L != 0: the rows run as Bluestein transforms
};

// grid ((H + 1) / 2, 3); dynamic LDS = 2 * lpad_size(max(W, bz.L)) complex.  Rows 2j (real part) and 2j+1 (imaginary part; the
// tail row of an odd H has none: zero), both reordered; the unpack of k_row_r2c_odd, no fold, no phase
template <int MODE>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_row_r2c_mirror(MirrorRowParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(max(p.W, p.bz.L));
    const int tid = threadIdx.x, T = blockDim.x;
    const int j = blockIdx.x, c = blockIdx.y;
    const int W = p.W;
    const bool two = 2 * j + 1 < p.H;                        // (workgroup-uniform)
    for (int n = tid; n < W; n += T)
        a[lpad(mirror_slot(n, W))] = make_float2((float)load_px<MODE>(p, c, 2 * j, n), two ? (float)load_px<MODE>(p, c, 2 * j + 1, n) : 0.f);
    __syncthreads();
    const float2* Z = fft_any<+1, 1>(a, b, p.plan, p.tw, p.bz, tid, T);
    // A = (Z[k] + conj Z[W-k]) / 2, B = (Z[k] - conj Z[W-k]) / 2i; k < ncols <= W/2 + 1
    const long tile_stride = (long)p.H * p.TK;
    float2* base = p.S1 + (long)c * p.NT * tile_stride;
    for (int k = tid; k < p.ncols; k += T) {
        const float2 zk = Z[lpad(k)];
        const float2 zn = Z[lpad(k == 0 ? 0 : W - k)];
        const float2 A = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
        const float2 B = make_float2(0.5f * (zk.y + zn.y), 0.5f * (-zk.x + zn.x));
        float2* dst = base + (long)(k / p.TK) * tile_stride + (long)(2 * j) * p.TK + (k % p.TK);
        dst[0] = A;
        if (two) dst[p.TK] = B;
    }
}

struct MirrorColParams {
    const float2* S1;        // blocked half spectrum, H rows, ncols columns
    float2* S2;              // the same columns, uH rows
    const float2* twH;
    StagePlan planH;
    int H, uH;
    int NT;
    int ncols;
    int kmax;                // kmax_y <= H
    BzPlan bzH;              // L != 0: the forward transform runs as a Bluestein transform
    CztPlan z;               // K = 2 kmax + 1, M = uH, the tables of period 2H
    const float2* rot;       // exp(+i pi k / 2H), k < H
};

// grid (NT, 3); dynamic LDS = 2 * lpad_size(max(H, bzH.L, z.L) * TK) complex.  The tile reordered along y, forward length H,
// Z_j = 2 C[|j - kmax|], chirp-z to uH points.
template <int TK>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_col_view_mirror(MirrorColParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(max(max(p.H, p.bzH.L), p.z.L) * TK);
    const int tid = threadIdx.x, T = blockDim.x;
    const int tile = blockIdx.x, c = blockIdx.y;
    const int H = p.H, uH = p.uH;
    const int ncol_valid = min(TK, p.ncols - tile * TK);
    const float2* src = p.S1 + ((long)c * p.NT + tile) * H * TK;
    for (int e = tid; e < H * TK; e += T) {
        const int y = e / TK, col = e % TK;
        float2 v = make_float2(0.f, 0.f);
        if (col < ncol_valid) v = src[e];
        a[lpad(mirror_slot(y, H) * TK + col)] = v;
    }
    __syncthreads();
    float2* F = fft_any<+1, TK>(a, b, p.planH, p.twH, p.bzH, tid, T);
    float2* G = (F == a) ? b : a;
    for (int e = tid; e < p.z.K * TK; e += T) {
        const int j = e / TK, col = e % TK;
        const int k = j < p.kmax ? p.kmax - j : j - p.kmax;
        float2 v = make_float2(0.f, 0.f);
        if (k < H) {                                         // (|f| = H: the zero bin of the extension)
            const float2 r = p.rot[k];
            v = cadd(cmul(cconj(r), F[lpad((k ? H - k : 0) * TK + col)]), cmul(r, F[lpad(k * TK + col)]));
        }
        G[lpad(e)] = v;
    }
    __syncthreads();
    const float2* D = fft_czt<TK>(G, F, p.z, tid, T);
    store_col_tile<TK>(p.S2 + ((long)c * p.NT + tile) * uH * TK, D, uH, ncol_valid, tid, T);
}

struct MirrorC2RParams {
    const float2* S2;        // blocked half spectrum after the column pass, uH rows, ncols columns
    void* R;                 // dense [3][uH][uW] float or half
    int W, uW, uH;
    int TK, NT;
    int kmax;                // kmax_x <= W
    CztPlan z;               // K = 2 kmax + 1, M = uW, the tables of period 2W
    const float2* rot;       // exp(+i pi k / 2W), k < W
};

// grid ((uH + 1) / 2, 3); dynamic LDS = 2 * lpad_size(z.L) complex.  Rows 2j and 2j+1: their cosine coefficients from the stored
// bins -- C[k] = Re(rot[k] U[k]) for 2k <= W, C[k] = Im(rot[W-k] U[W-k]) above -- as Z_f = 2 (C_A[|f|] + i C_B[|f|]): the map is
// real, so the real part of the result is row 2j and the imaginary part row 2j+1.  The tail row of an odd uH has no partner.
template <bool HALF_OUT>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_row_view_c2r_mirror(MirrorC2RParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(p.z.L);
    const int tid = threadIdx.x, T = blockDim.x;
    const int j = blockIdx.x, c = blockIdx.y;
    const int W = p.W, uW = p.uW;
    const bool two = 2 * j + 1 < p.uH;                       // (workgroup-uniform)
    const long tile_stride = (long)p.uH * p.TK;
    const float2* baseA = p.S2 + (long)c * p.NT * tile_stride + (long)(2 * j) * p.TK;
    const float2* baseB = baseA + p.TK;                      // (read only when the row exists)
    for (int k = tid; k <= p.kmax; k += T) {
        float2 v = make_float2(0.f, 0.f);
        if (k < W) {                                         // (|f| = W: the zero bin of the extension)
            const bool low = 2 * k <= W;
            const int kk = low ? k : W - k;
            const long o = (long)(kk / p.TK) * tile_stride + (kk % p.TK);
            const float2 r = p.rot[kk];
            const float2 A = cmul(r, baseA[o]);
            const float2 B = two ? cmul(r, baseB[o]) : make_float2(0.f, 0.f);
            v = low ? make_float2(2.f * A.x, 2.f * B.x) : make_float2(2.f * A.y, 2.f * B.y);
        }
        a[lpad(p.kmax - k)] = v;
        if (k) a[lpad(p.kmax + k)] = v;
    }
    __syncthreads();
    const float2* zz = fft_czt<1>(a, b, p.z, tid, T);
    const long plane = (long)uW * p.uH, row = c * plane + (long)(2 * j) * uW;
    for (int n = tid; n < uW; n += T) {
        const float2 v = zz[lpad(n)];
        store_px<HALF_OUT>(p.R, row, n, v.x);
        if (two) store_px<HALF_OUT>(p.R, row, uW + n, v.y);
    }
}

}  // namespace fftup
