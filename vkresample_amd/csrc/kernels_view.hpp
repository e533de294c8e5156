// kernels_view.hpp -- view plans (fftup_plan_create_view, include/fftup.h): zoom and pan at any real ratio.
//
// Per axis, separable: the frame's trigonometric interpolant, evaluated at the M positions t_m = origin + m s (s = span / M, pixel
// indices as coordinates, the frame periodic with period N).  With X = DFT_N(x), kmax = min(N/2, floor(N M / (2 max(span, M)))):
//     y[m] = (1/N) sum_{f = -kmax .. kmax} g_f X[f mod N] exp(2 pi i f t_m / N),     g_f = 1/2 where 2 |f| == N, else 1.
// The K = 2 kmax + 1 bins go in at j = f + kmax.  With theta = 2 pi / N and j m = (j^2 + m^2 - (m - j)^2) / 2 this is a chirp-z
// transform with a free rate (fft_bluestein, kernels_bluestein.hpp, is the same thing with the rate pinned to 1/N):
//     y[m] = post[m] * sum_j (Z_j pre[j]) c[m - j]
// -- a convolution, run as a cyclic one of a 2,3,5,7-smooth length L >= K + M - 1 through the Stockham stages that exist:
//     a[j] = Z_j pre[j] (zero up to L),  A = FFT_L(a),  A[k] *= bhat[k],  r = IFFT_L(A),  y[m] = r[m] post[m].
// The tables come from the host (view_tables.hpp: long double phases, reduced before the multiplication by pi, rounded once to
// fp32) or, for a frame that brings its own view, from k_view_tables (kernels_view_tables.hpp); post carries the normalisation (1/N) (span/M) of the pre-sharpen image R = y span_x span_y / (uW uH).
//
// The forward transforms of these plans run with exp(+2 pi i nk / N) (fft_any<+1>), as in kernels_odd.hpp: bin k of the kernels holds
// the frequency -k.  The gathers below read Z_j = X[f] from kernel bin -f = kmax - j.
// A frame is k_row_r2c_odd (kernels_odd.hpp, unchanged: kmax = kmax_x, no fold, no phase table) -> k_col_view -> k_row_view_c2r ->
// the sharpen pass.  New parameter structs live here: kernels_generic.hpp and its neighbours are embedded for the plan-time
// compiler and fingerprinted by the committed counter profiles, and stay byte-identical.  fp32 arithmetic only (-p 0 and -p 2).
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "bluestein_plan.hpp"
#include "fft_engine.hpp"
#include "kernels_bluestein.hpp"
#include "kernels_generic.hpp"

namespace fftup {

struct CztPlan {
    int32_t L;               // convolution length (smooth, >= K + M - 1; fixed by N and M: >= 2 (N/2) + M)
    int32_t K, M;            // bins in (2 kmax + 1), points out
    StagePlan plan;          // n = L
    const float2* tw;        // L-th roots, exp(+2 pi i k / L)
    const float2* pre;       // K points
    const float2* post;      // M points
    const float2* bhat;      // FFT_L(c wrapped) / L, L points
};

// The calling shape of fft_bluestein: TK interleaved sequences of K points Z_j in `a` as complex [j][TK] (valid after a barrier
// executed by the caller), both buffers hold lpad_size(z.L * TK) points; returns the buffer holding the M * TK results (synced).
template <int TK>
__device__ __forceinline__ float2* fft_czt(float2* a, float2* b, const CztPlan& z, int tid, int T)
{
    const int L = z.L;
    for (int e = tid; e < L * TK; e += T) {
        const int j = e / TK;
        float2 v = make_float2(0.f, 0.f);
        if (j < z.K) v = cmul(a[lpad(e)], z.pre[j]);
        a[lpad(e)] = v;
    }
    __syncthreads();
    float2* A = fft_lds<+1, TK>(a, b, z.plan, z.tw, tid, T);
    float2* B = (A == a) ? b : a;
    for (int e = tid; e < L * TK; e += T) A[lpad(e)] = cmul(A[lpad(e)], z.bhat[e / TK]);
    __syncthreads();
    float2* r = fft_lds<-1, TK>(A, B, z.plan, z.tw, tid, T);
    for (int e = tid; e < z.M * TK; e += T) r[lpad(e)] = cmul(r[lpad(e)], z.post[e / TK]);
    __syncthreads();
    return r;
}

struct ViewColParams {
    const float2* S1;        // blocked half spectrum, H rows, kmax_x + 1 columns
    float2* S2;              // the same columns, uH rows
    const float2* twH;
    StagePlan planH;
    int H, uH;
    int NT;
    int ncols;               // kx columns present: kmax_x + 1
    int kmax;                // kmax_y <= H/2
    BzPlan bzH;              // L != 0: the forward transform runs as a Bluestein transform
    CztPlan z;               // K = 2 kmax + 1, M = uH
};

// grid (NT, 3); dynamic LDS = 2 * lpad_size(max(H, bzH.L, z.L) * TK) complex.  Forward length H, the signed bins -kmax .. kmax,
// chirp-z to uH points.
template <int TK>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_col_view(ViewColParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(max(max(p.H, p.bzH.L), p.z.L) * TK);
    const int tid = threadIdx.x, T = blockDim.x;
    const int tile = blockIdx.x, c = blockIdx.y;
    const int H = p.H, uH = p.uH;
    const int ncol_valid = min(TK, p.ncols - tile * TK);
    load_col_tile<TK>(a, p.S1 + ((long)c * p.NT + tile) * H * TK, H, ncol_valid, tid, T);
    __syncthreads();
    float2* F = fft_any<+1, TK>(a, b, p.planH, p.twH, p.bzH, tid, T);
    float2* G = (F == a) ? b : a;
    // Z_j = X[j - kmax] sits in kernel bin kmax - j (mod H); kmax <= H/2: the Nyquist bin of an even H is read from both ends
    for (int e = tid; e < p.z.K * TK; e += T) {
        const int j = e / TK, col = e % TK;
        int k = p.kmax - j;
        if (k < 0) k += H;
        G[lpad(e)] = F[lpad(k * TK + col)];
    }
    __syncthreads();
    const float2* D = fft_czt<TK>(G, F, p.z, tid, T);
    store_col_tile<TK>(p.S2 + ((long)c * p.NT + tile) * uH * TK, D, uH, ncol_valid, tid, T);
}

struct ViewC2RParams {
    const float2* S2;        // blocked half spectrum after the column pass, uH rows, kmax + 1 columns
    void* R;                 // dense [3][uH][uW] float or half
    int uW, uH;
    int TK, NT;
    int kmax;                // kmax_x
    CztPlan z;               // K = 2 kmax + 1, M = uW
};

// grid ((uH + 1) / 2, 3); dynamic LDS = 2 * lpad_size(z.L) complex.  Rows 2j and 2j+1 of the spectrum as one complex sequence:
// kernel bin k holds A + iB, kernel bin -k holds conj(A) + i conj(B) (the two rows are real), k = 0 .. kmax; the tail row of an
// odd uH has no partner: B = 0, one row out.  The real part of the result is row 2j, the imaginary part row 2j+1.
template <bool HALF_OUT>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_row_view_c2r(ViewC2RParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(p.z.L);
    const int tid = threadIdx.x, T = blockDim.x;
    const int j = blockIdx.x, c = blockIdx.y;
    const int uW = p.uW;
    const bool two = 2 * j + 1 < p.uH;                       // (workgroup-uniform)
    const long tile_stride = (long)p.uH * p.TK;
    const float2* baseA = p.S2 + (long)c * p.NT * tile_stride + (long)(2 * j) * p.TK;
    const float2* baseB = baseA + p.TK;                      // (read only when the row exists)
    for (int k = tid; k <= p.kmax; k += T) {
        const long o = (long)(k / p.TK) * tile_stride + (k % p.TK);
        const float2 A = baseA[o];
        const float2 B = two ? baseB[o] : make_float2(0.f, 0.f);
        a[lpad(p.kmax - k)] = make_float2(A.x - B.y, A.y + B.x);
        if (k) a[lpad(p.kmax + k)] = make_float2(A.x + B.y, -A.y + B.x);
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
