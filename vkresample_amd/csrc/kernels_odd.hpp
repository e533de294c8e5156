// kernels_odd.hpp -- the resampling kernels.  Written for FFTUP_FLAG_ODD_SIZE (include/fftup.h): plans with an odd width or height,
// input or output; the rule below covers every parity and direction, so these kernels also run
//   * the plans of fftup_plan_create_size (either direction per axis, centre alignment: the phase tables);
//   * the forward rows of a size-generic FFTUP_FLAG_ANY_SIZE plan whose width needs a Bluestein transform: k_row_r2c_odd with
//     kmax = W/2 and no fold is the size-generic unpack (its columns and inverse rows keep the reference's shift, read guard and
//     doubled Nyquist bin: k_col_bz / k_row_c2r_bz, kernels_bluestein.hpp);
//   * the forward rows of fftup_plan_create_view (kernels_view.hpp).
// FFT downscale plans with four even lengths keep kernels of their own (kernels_downscale.hpp: the same rule with uW < W, uH < H written
// out): on these kernels their 4096x2048 -> 2048x1024 frame measured 1.7 to 2.7 % slower, profiles/resample_kernels_ab.json.
//
// Such a plan computes exact trigonometric resampling per axis (scipy.signal.resample's rule), separably.  Per axis, for an input
// of N points with spectrum X = DFT_N(x), an output of M points and K = min(N, M):
//     bins |k| < K/2 are copied,            Y[k mod M] = X[k mod N];
//     K even, its Nyquist bin h = K/2:      M > N: split, Y[h] = Y[M-h] = X[h]/2;   M < N: folded, Y[h] = X[h] + X[N-h];   M = N: kept;
//     every other bin of Y is 0,
// and R = (1/M) IDFT_M(Y).  The quirks B1-B3 of the reference's even-size path (its read guard, its doubled Nyquist bin) do not
// apply on either axis.  An odd length has no Nyquist bin: its bins pair up as k and N - k for k = 1 .. (N-1)/2 and nothing else.
//
// The three kernels are the size-generic row R2C, column and row C2R kernels (kernels_generic.hpp / kernels_bluestein.hpp) -- same
// blocked half spectrum S[c][tile][ky][TK], same two-real-rows-as-one-complex packing, every transform chosen per transform by
// fft_any (Stockham stages for a 2,3,5,7-smooth length, radices 3/5/7 only when it is odd; Bluestein otherwise) -- with
//   * the TAIL ROW: an odd number of rows leaves one row without a partner.  The grid has (rows + 1) / 2 workgroups; the last one
//     transforms its single row with a zero imaginary part and reads / writes one spectrum row and one image row.
//   * the half spectrum holds kx = 0 .. min(W, uW)/2 (floor): W/2 + 1 columns of an odd W, none of them self-paired.
//   * the bin map above instead of the reference's shift and read guard; the zero rows and columns are never stored.
//   * scalar stores of the binary16 image: with an odd uW every second row of a plane starts on a 2-byte boundary only.
// CENTRE ALIGNMENT (fftup_plan_create_size, FFTUP_ALIGN_CENTRE): per axis N -> M the output pixel m sits at input position
// (m + 1/2) N / M - 1/2 instead of m N / M -- a shift by d = (N/M - 1)/2 input pixels, i.e. the factor exp(+2 pi i f d / N) on the bin
// of signed frequency f of the DFT with exp(-2 pi i nk / N).  The forward transforms here run with exp(+2 pi i nk / N) (fft_any<+1>),
// so bin k of these kernels holds the frequency -k: the table `ph` of an axis holds ph[k] = exp(-2 pi i k d / N), k = 0 .. min(N, M)/2,
// the factor of kernel bin +k; bin -k takes its conjugate.  The split Nyquist bin keeps its two different halves, X[h] ph[h] / 2 and
// X[h] conj(ph[h]) / 2, the folded one becomes X[h] ph[h] + X[N-h] conj(ph[h]).  ph == nullptr (corner alignment, or M == N):
// nothing is multiplied, the kernels compute what they computed before the table existed.
// New parameter structs live here: kernels_generic.hpp and its neighbours are embedded for the plan-time compiler and
// fingerprinted by the committed counter profiles, and stay byte-identical.  fp32 arithmetic only (-p 0 and -p 2).
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "bluestein_plan.hpp"
#include "fft_engine.hpp"
#include "kernels_bluestein.hpp"
#include "kernels_generic.hpp"

namespace fftup {

struct OddRowParams {
    const void* in;          // planar float/half (row stride, plane stride in elements) or u8 RGB (row stride bytes)
    float2* S1;              // blocked half spectrum, H rows, kmax + 1 columns
    const float2* tw;        // W-th roots (direct transform)
    StagePlan plan;          // n = W
    int W, H;
    long in_row_stride, in_plane_stride;
    int TK, NT;              // tile width (complex), number of tiles = ceil((kmax + 1) / TK)
    int kmax;                // the last bin kept: min(W, uW) / 2
    int fold;                // 1: uW < W and uW even -- bin kmax is the output's Nyquist bin, stored folded: X[h] + X[W-h] = 2 Re X[h]
    BzPlan bz;               // L != 0: the rows run as Bluestein transforms
    const float2* ph;        // centre alignment: kmax + 1 phase factors (see above), or nullptr
};

__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }

// grid ((H + 1) / 2, 3); dynamic LDS = 2 * lpad_size(max(W, bz.L)) complex.  Rows 2j (real part) and 2j+1 (imaginary part; the
// tail row of an odd H has none: zero)
template <int MODE>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_row_r2c_odd(OddRowParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(max(p.W, p.bz.L));
    const int tid = threadIdx.x, T = blockDim.x;
    const int j = blockIdx.x, c = blockIdx.y;
    const int W = p.W;
    const bool two = 2 * j + 1 < p.H;                        // (workgroup-uniform)
    for (int n = tid; n < W; n += T)
        a[lpad(n)] = make_float2((float)load_px<MODE>(p, c, 2 * j, n), two ? (float)load_px<MODE>(p, c, 2 * j + 1, n) : 0.f);
    __syncthreads();
    const float2* Z = fft_any<+1, 1>(a, b, p.plan, p.tw, p.bz, tid, T);
    // unpack as k_row_r2c: A = (Z[k] + conj Z[W-k]) / 2, B = (Z[k] - conj Z[W-k]) / 2i.  k <= kmax <= W/2 (floor): for an odd W
    // the partner W - k is never k itself
    const long tile_stride = (long)p.H * p.TK;
    float2* base = p.S1 + (long)c * p.NT * tile_stride;
    for (int k = tid; k <= p.kmax; k += T) {
        const float2 zk = Z[lpad(k)];
        const float2 zn = Z[lpad(k == 0 ? 0 : W - k)];
        float2 A = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
        float2 B = make_float2(0.5f * (zk.y + zn.y), 0.5f * (-zk.x + zn.x));
        // (both rows are real: their bins take the same factor, and the folded bin X[h] w + conj(X[h] w) stays 2 Re)
        if (p.ph) { const float2 w = p.ph[k]; A = cmul(A, w); B = cmul(B, w); }
        if (p.fold && k == p.kmax) { A = make_float2(2.f * A.x, 0.f); B = make_float2(2.f * B.x, 0.f); }
        float2* dst = base + (long)(k / p.TK) * tile_stride + (long)(2 * j) * p.TK + (k % p.TK);
        dst[0] = A;
        if (two) dst[p.TK] = B;
    }
}

struct OddColParams {
    const float2* S1;
    float2* S2;
    const float2 *twH, *twUH;
    StagePlan planH, planUH;
    int H, uH;
    int NT;
    int ncols;               // kx columns present: min(W, uW)/2 + 1
    float inv_norm;          // 1/uH
    BzPlan bzH, bzUH;        // per transform, L = 0 for a smooth length
    const float2* ph;        // centre alignment: min(H, uH)/2 + 1 phase factors (see above), or nullptr
};

// grid (NT, 3); dynamic LDS = 2 * lpad_size(max(H, uH, bzH.L, bzUH.L) * TK) complex.  Forward length H, the bin map, inverse length
// uH -- either parity, uH above, below or equal to H.
template <int TK>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_col_odd(OddColParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(max(max(p.H, p.uH), max(p.bzH.L, p.bzUH.L)) * TK);
    const int tid = threadIdx.x, T = blockDim.x;
    const int tile = blockIdx.x, c = blockIdx.y;
    const int H = p.H, uH = p.uH, K = min(H, uH);
    const int ncol_valid = min(TK, p.ncols - tile * TK);
    load_col_tile<TK>(a, p.S1 + ((long)c * p.NT + tile) * H * TK, H, ncol_valid, tid, T);
    __syncthreads();
    float2* F = fft_any<+1, TK>(a, b, p.planH, p.twH, p.bzH, tid, T);
    float2* G = (F == a) ? b : a;
    // output bin ky holds the frequency f = ky (2 ky < uH) or ky - uH; its source is bin f mod H
    for (int e = tid; e < uH * TK; e += T) {
        const int ky = e / TK, col = e % TK;
        const int f = 2 * ky < uH ? ky : ky - uH, af = f < 0 ? -f : f;
        float2 v = make_float2(0.f, 0.f);
        if (2 * af < K) {
            v = F[lpad((f < 0 ? H + f : f) * TK + col)];
            if (p.ph) v = cmul(v, f < 0 ? cconj(p.ph[af]) : p.ph[af]);
        }
        else if (2 * af == K) {                                          // the Nyquist bin of the shorter, even length
            float2 lo = F[lpad(af * TK + col)];
            if (uH > H) {                                                // split: ky = H/2 and ky = uH - H/2
                if (p.ph) lo = cmul(lo, f < 0 ? cconj(p.ph[af]) : p.ph[af]);
                v = cscale(lo, 0.5f);
            }
            else if (uH < H) {                                           // folded (ky = uH/2 only)
                float2 hi = F[lpad((H - af) * TK + col)];
                if (p.ph) { lo = cmul(lo, p.ph[af]); hi = cmul(hi, cconj(p.ph[af])); }
                v = cadd(lo, hi);
            }
            else v = lo;
        }
        G[lpad(e)] = v;
    }
    __syncthreads();
    const float2* D = fft_any<-1, TK>(G, F, p.planUH, p.twUH, p.bzUH, tid, T);
    store_col_tile<TK>(p.S2 + ((long)c * p.NT + tile) * uH * TK, D, uH, ncol_valid, p.inv_norm, tid, T);
}

struct OddC2RParams {
    const float2* S2;        // blocked half spectrum after the column pass, uH rows, kmax + 1 columns
    void* R;                 // dense [3][uH][uW] float or half
    const float2* tw;        // uW-th roots (direct transform)
    StagePlan plan;          // n = uW
    int uW, uH;
    int TK, NT;
    int kmax;                // the last bin the spectrum holds: min(W, uW) / 2
    int halve;               // 1: uW > W and W even -- bin kmax is the input's Nyquist bin, split: Y[h] = Y[uW-h] = X[h] / 2 (with centre
                             // alignment it carries its phase, X[h] ph[h]: the loop below writes bin uW - h as its conjugate, as for any k)
    float inv_norm;          // 1/uW
    BzPlan bz;               // L != 0: the rows run as Bluestein transforms
};

// grid ((uH + 1) / 2, 3); dynamic LDS = 2 * lpad_size(max(uW, bz.L)) complex.  Rows 2j and 2j+1 of the spectrum as one complex row
// Z[k] = A + iB, Z[uW-k] = conj(A) + i conj(B) for k = 1 .. (uW-1)/2; the self-conjugate bin uW/2 exists for an even uW only (and
// is non-zero only when the spectrum reaches it: uW <= W).  The tail row of an odd uH has no partner: B = 0, one row out.
template <bool HALF_OUT>
__global__ void __launch_bounds__(GenericMaxThreads<float2>::value) k_row_c2r_odd(OddC2RParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* a = (float2*)smem;
    float2* b = a + lpad_size(max(p.uW, p.bz.L));
    const int tid = threadIdx.x, T = blockDim.x;
    const int j = blockIdx.x, c = blockIdx.y;
    const int uW = p.uW;
    const bool two = 2 * j + 1 < p.uH;                       // (workgroup-uniform)
    const long tile_stride = (long)p.uH * p.TK;
    const float2* baseA = p.S2 + (long)c * p.NT * tile_stride + (long)(2 * j) * p.TK;
    const float2* baseB = baseA + p.TK;                      // (read only when the row exists)
    const float2 zero = make_float2(0.f, 0.f);
    for (int k = 1 + tid; k <= (uW - 1) / 2; k += T) {
        float2 A = zero, B = zero;
        if (k <= p.kmax) {
            const long o = (long)(k / p.TK) * tile_stride + (k % p.TK);
            A = baseA[o];
            if (two) B = baseB[o];
            if (p.halve && k == p.kmax) { A = cscale(A, 0.5f); B = cscale(B, 0.5f); }
        }
        a[lpad(k)] = make_float2(A.x - B.y, A.y + B.x);
        a[lpad(uW - k)] = make_float2(A.x + B.y, -A.y + B.x);
    }
    if (tid == 0) {
        const float2 A = baseA[0], B = two ? baseB[0] : zero;
        a[lpad(0)] = make_float2(A.x - B.y, A.y + B.x);
        if (!(uW & 1)) {
            const int h = uW / 2;
            float2 Ah = zero, Bh = zero;
            if (h <= p.kmax) {
                const long o = (long)(h / p.TK) * tile_stride + (h % p.TK);
                Ah = baseA[o];
                if (two) Bh = baseB[o];
            }
            a[lpad(h)] = make_float2(Ah.x - Bh.y, Ah.y + Bh.x);
        }
    }
    __syncthreads();
    const float2* zz = fft_any<-1, 1>(a, b, p.plan, p.tw, p.bz, tid, T);
    const long plane = (long)uW * p.uH, row = c * plane + (long)(2 * j) * uW;
    for (int n = tid; n < uW; n += T) {
        const float2 v = cscale(zz[lpad(n)], p.inv_norm);
        store_px<HALF_OUT>(p.R, row, n, v.x);
        if (two) store_px<HALF_OUT>(p.R, row, uW + n, v.y);
    }
}

// fftup_output_checksum over an output that is no whole number of 32-bit words (binary16 planes with uW uH odd): the trailing
// `n` (1..3) bytes enter the sum as one little-endian word, zero-extended.  One thread.
__global__ void __launch_bounds__(64) k_checksum_tail(const uint8_t* __restrict__ bytes, int n, unsigned long long* sum)
{
    if (blockIdx.x || threadIdx.x) return;
    unsigned w = 0;
    for (int i = 0; i < n; i++) w |= (unsigned)bytes[i] << (8 * i);
    atomicAdd(sum, (unsigned long long)w);
}

}  // namespace fftup
