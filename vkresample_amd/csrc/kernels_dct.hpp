// kernels_dct.hpp -- size-generic HIP kernels of the DCT upscale mode (FFTUP_FLAG_DCT, include/fftup.h): DCT-II -> zero-pad ->
// DCT-III per axis instead of R2C FFT -> centred pad -> C2R.  Three launches per frame, then the FFT path's sharpen pass:
//   k_dct_row    DCT-II of the rows (pairs of rows)                                   input -> S1 real [3][H][W]
//   k_dct_col    DCT-II of the columns, zero-pad, DCT-III of length uH (column pairs)  S1 -> S2 real [3][uH][W]
//   k_idct_row   DCT-III of length uW of the rows (pairs of rows)                      S2 -> R dense [3][uH][uW], R = y / upsq
// Every DCT is one complex FFT of the LDS Stockham engine (fft_engine.hpp) of the same length (Makhoul):
//   DCT-II   v[n] = x[2n], v[N-1-n] = x[2n+1];  X[k] = Re(exp(-i pi k / 2N) FFT(v)[k])          (FFT: exp(-2 pi i nk/N), DIR = -1)
//   DCT-III  W[0] = C[0], W[k] = 1/2 exp(i pi k / 2M) (C[k] - i C[M-k]);  w[n] = sum_k W[k] exp(+2 pi i kn/M) is real (DIR = +1);
//            y[2n] = w[n], y[2n+1] = w[M-1-n]
// with C[0] = X[0]/N, C[k] = 2 X[k]/N (k < N), 0 beyond.  Two real sequences a, b ride in one complex transform: z = a + i b
// forward, separated by Hermitian symmetry (Z[k] +- conj Z[N-k]); W_a + i W_b inverse, w_a and w_b come out as its real and
// imaginary parts.  For k >= 1 the pair's inverse input is
//   W[k] = (1/N) exp(i pi k / 2M) ((Xa[k] + Xb[M-k]) + i (Xb[k] - Xa[M-k]))       (X[j] = 0 for j >= N)
// The rotations exp(i pi k / 2n) come from host tables computed in double, rounded once to fp32, as the FFT twiddles.
// Sizes: N, M even (the plan's rule).  fp32 arithmetic; -p 2 stores R as binary16.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "fft_engine.hpp"
#include "kernels_generic.hpp"

namespace fftup {

// (Xa, Xb) of one pair from the forward FFT Z of a + i b at k: zk = Z[k], zn = Z[(N-k) mod N], r = exp(i pi k / 2N)
__device__ __forceinline__ float2 dct2_unpack(float2 zk, float2 zn, float2 r)
{
    // Va = (Z[k] + conj Z[N-k]) / 2, Vb = (Z[k] - conj Z[N-k]) / 2i, X = Re(conj(r) V) = r.x V.x + r.y V.y
    const float2 va = make_float2(zk.x + zn.x, zk.y - zn.y), vb = make_float2(zk.y + zn.y, zn.x - zk.x);
    return make_float2(0.5f * fmaf(r.x, va.x, r.y * va.y), 0.5f * fmaf(r.x, vb.x, r.y * vb.y));
}
// W[k] (k >= 1) of the pair from xk = (Xa, Xb)[k] and xm = (Xa, Xb)[M-k] (zero beyond N), r = exp(i pi k / 2M), s = 1/N
__device__ __forceinline__ float2 dct3_pack(float2 xk, float2 xm, float2 r, float s)
{
    const float2 p = make_float2(s * (xk.x + xm.y), s * (xk.y - xm.x));
    return cmul(r, p);
}

struct DctRowParams {
    const void* in;          // planar float/half (row stride, plane stride in elements) or u8 RGB (row stride bytes)
    float* S1;               // real coefficients [3][H][W]
    const float2* tw;        // W-th roots (FFT twiddles)
    const float2* rot;       // exp(i pi k / 2W), k < W
    StagePlan plan;          // n = W
    int W, H;
    long in_row_stride, in_plane_stride;
};

// grid (H/2, 3); dynamic LDS = 2 * lpad_size(W) complex.  Rows 2j (real part) and 2j+1 (imaginary part).
template <int MODE>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_dct_row(DctRowParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(p.W);
    const int tid = threadIdx.x, T = blockDim.x;
    const int j = blockIdx.x, c = blockIdx.y;
    const int W = p.W;
    for (int x = tid; x < W; x += T) {                     // pixel x -> v[x/2] (even x), v[W-1-x/2] (odd x)
        const int n = (x & 1) ? W - 1 - (x >> 1) : (x >> 1);
        a[lpad(n)] = make_float2((float)load_px<MODE>(p, c, 2 * j, x), (float)load_px<MODE>(p, c, 2 * j + 1, x));
    }
    __syncthreads();
    const float2* Z = fft_lds<-1, 1>(a, b, p.plan, p.tw, tid, T);
    float* ra = p.S1 + ((long)c * p.H + 2 * j) * W;
    for (int k = tid; k < W; k += T) {
        const float2 x = dct2_unpack(Z[lpad(k)], Z[lpad(k == 0 ? 0 : W - k)], p.rot[k]);
        ra[k] = x.x;
        ra[W + k] = x.y;
    }
}

struct DctColParams {
    const float* S1;         // [3][H][W]
    float* S2;               // [3][uH][W]
    const float2 *twH, *twUH;
    const float2 *rotH, *rotUH;    // exp(i pi k / 2H), k < H; exp(i pi k / 2uH), k < uH
    StagePlan planH, planUH;
    int W, H, uH;
    float inv_norm;          // 1/H
};

// grid (ceil(W/2 / TK), 3); dynamic LDS = 2 * lpad_size(max(H, uH)*TK) complex.  Sequence col of tile t: the real columns 2q, 2q+1,
// q = t TK + col, as one complex sequence -- TK pairs = 2 TK floats = 8 TK contiguous bytes of every row read and written.
// Downscale plans (uH < H, FFTUP_FLAG_DOWNSCALE): the DCT-III below reads the coefficients k < uH only -- truncation instead of
// zero-padding, with the same loops.
template <int TK>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_dct_col(DctColParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(max(p.H, p.uH) * TK);
    const int tid = threadIdx.x, T = blockDim.x;
    const int tile = blockIdx.x, c = blockIdx.y;
    const int W = p.W, H = p.H, uH = p.uH;
    const int npairs = min(TK, W / 2 - tile * TK);
    const float* src = p.S1 + (long)c * H * W + 2 * tile * TK;
    for (int e = tid; e < H * TK; e += T) {
        const int r = e / TK, col = e % TK;              // source row r -> v[r/2] (even r), v[H-1-r/2] (odd r)
        const int n = (r & 1) ? H - 1 - (r >> 1) : (r >> 1);
        float2 v = make_float2(0.f, 0.f);
        if (col < npairs) v = *(const float2*)(src + (long)r * W + 2 * col);
        a[lpad(n * TK + col)] = v;
    }
    __syncthreads();
    float2* F = fft_lds<-1, TK>(a, b, p.planH, p.twH, tid, T);
    float2* G = (F == a) ? b : a;
    for (int e = tid; e < H * TK; e += T) {
        const int k = e / TK, col = e % TK;
        G[lpad(e)] = dct2_unpack(F[lpad(e)], F[lpad((k == 0 ? 0 : H - k) * TK + col)], p.rotH[k]);
    }
    __syncthreads();
    // the DCT-III input of length uH (F is free again: its FFT has been unpacked into G)
    for (int e = tid; e < uH * TK; e += T) {
        const int k = e / TK, col = e % TK;
        float2 w;
        if (k == 0) {
            const float2 x0 = G[lpad(col)];
            w = make_float2(p.inv_norm * x0.x, p.inv_norm * x0.y);
        } else {
            const float2 xk = k < H ? G[lpad(e)] : make_float2(0.f, 0.f);
            const float2 xm = uH - k < H ? G[lpad((uH - k) * TK + col)] : make_float2(0.f, 0.f);
            w = dct3_pack(xk, xm, p.rotUH[k], p.inv_norm);
        }
        F[lpad(e)] = w;
    }
    __syncthreads();
    const float2* D = fft_lds<+1, TK>(F, G, p.planUH, p.twUH, tid, T);
    float* dst = p.S2 + (long)c * uH * W + 2 * tile * TK;
    for (int e = tid; e < uH * TK; e += T) {
        const int m = e / TK, col = e % TK;              // y[m] = w[m/2] (even m), w[uH-1-m/2] (odd m)
        const int n = (m & 1) ? uH - 1 - (m >> 1) : (m >> 1);
        if (col < npairs) *(float2*)(dst + (long)m * W + 2 * col) = D[lpad(n * TK + col)];
    }
}

struct IdctRowParams {
    const float* S2;         // [3][uH][W]
    void* R;                 // dense [3][uH][uW] float or half
    const float2* tw;        // uW-th roots
    const float2* rot;       // exp(i pi k / 2uW), k < uW
    StagePlan plan;          // n = uW
    int W, uW, uH;
    float inv_norm;          // 1 / (W upsq): the DCT-III's 1/W and the pre-sharpen convention R = y / upsq in one constant
};

// grid (uH/2, 3); dynamic LDS = 2 * lpad_size(uW) complex.  Rows 2j (real part) and 2j+1 (imaginary part).  Downscale plans
// (uW < W): only the coefficients k < uW are loaded -- the DCT-III reads no others, and b holds lpad_size(uW) points.
template <bool HALF_OUT>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_idct_row(IdctRowParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(p.uW);
    const int tid = threadIdx.x, T = blockDim.x;
    const int j = blockIdx.x, c = blockIdx.y;
    const int W = p.W, uW = p.uW;
    const float* ra = p.S2 + ((long)c * p.uH + 2 * j) * W;
    for (int k = tid; k < min(W, uW); k += T) b[lpad(k)] = make_float2(ra[k], ra[W + k]);
    __syncthreads();
    for (int k = tid; k < uW; k += T) {
        float2 w;
        if (k == 0) w = b[lpad(0)];
        else {
            const float2 xk = k < W ? b[lpad(k)] : make_float2(0.f, 0.f);
            const float2 xm = uW - k < W ? b[lpad(uW - k)] : make_float2(0.f, 0.f);
            w = dct3_pack(xk, xm, p.rot[k], 1.0f);
        }
        a[lpad(k)] = w;
    }
    __syncthreads();
    const float2* z = fft_lds<+1, 1>(a, b, p.plan, p.tw, tid, T);
    const long plane = (long)uW * p.uH;
    for (int m = tid; m < uW; m += T) {
        const int n = (m & 1) ? uW - 1 - (m >> 1) : (m >> 1);
        const float2 v = cscale(z[lpad(n)], p.inv_norm);
        if constexpr (HALF_OUT) {
            __half* R = (__half*)p.R + c * plane + (long)(2 * j) * uW;
            R[m] = __float2half_rn(v.x);
            R[uW + m] = __float2half_rn(v.y);
        } else {
            float* R = (float*)p.R + c * plane + (long)(2 * j) * uW;
            R[m] = v.x;
            R[uW + m] = v.y;
        }
    }
}

}  // namespace fftup
