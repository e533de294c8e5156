// kernels_roll.hpp -- roll estimates (include/fftup.h, fftup_roll_angles): the rotation between two frames from the magnitudes of
// their spectra, sampled on a polar grid and correlated along the angle, phase only, with a sub-sample refinement.  Four kernels per
// chunk of pairs, the pair in blockIdx.z, nothing read by the host in between:
//   k_roll_rows   one workgroup per window row: step 1 of the aligner for BOTH frames (align_window_px), z = a + i b in the first
//                 n_x of 2 n_x points of LDS, the rest zeros; forward row transform; only the band's columns -cx - 1 .. cx + 1 go to HBM
//   k_roll_cols   one workgroup per column PAIR (k_x, -k_x) of the band, side by side in LDS (TK = 2) as in k_align_cols: the n_y
//                 rows that are not zero, padded to 2 n_y; forward column transforms; A / B separated from Z[k] and conj Z[-k] (the
//                 partner bin lives in the other column of the pair); (log1p |A|, log1p |B|) of rows 0 .. cy + 1 to HBM
//   k_roll_polar  one workgroup per radius: the n_theta bilinear samples of both log-magnitudes as two interleaved sequences in
//                 LDS, their transforms, F^B conj F^A for m = 1 .. m_b to HBM (the profiles are real: bin -m is the conjugate)
//   k_roll_peak   one workgroup per pair: the sum over the radii in one fixed order, R = P / |P| with the floor rule, the Hermitian
//                 spectrum in LDS, inverse transform, coarse argmax; the interpolant on 2 kappa + 1 points (fp64 sums, the phases
//                 from a table of the (kappa n_theta)-th roots by integer arithmetic, as the aligner's fine stage), argmax, parabola,
//                 one 16-byte store of the fftup_roll_angle
// No atomics; every store is a plain vector store.  Transform direction: fft_engine's DIR = -1 is numpy's forward DFT.
// LDS: rows 2 lpad(2 n_x) float2 (17.4 KB at n_x = 512); columns 2 lpad(4 n_y) float2 (34.8 KB at n_y = 512); polar 2 lpad(2 n_theta)
// float2 (34.8 KB at 1024 angles); peak 2 lpad(n_theta) float2 and 3.6 KB static.  At 256 threads a compute unit holds four such
// workgroups.  Not handed to the plan-time compiler.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_align.hpp"

namespace fftup {

constexpr int ROLL_MAX_MB = 256;                  // m_b = n_theta / 4 at 1024 angles
constexpr int ROLL_MAX_FINE = 129;                // 2 kappa + 1 at kappa = 64

struct RollParams {
    int nx, ny, d, crop_x, crop_y, kappa, nt, rho_min, nrho, mb, cx, cy, ncol, nrow, sx, sy;   // ncol = 2 cx + 3, nrow = cy + 2; sx = n_x / n
    StagePlan planX, planY, planT;  // 2 n_x, 2 n_y, n_theta points
    const float2 *twX, *twY, *twT;  // their roots exp(+2 pi i k / N)
    const float *winX, *winY;       // w[n] = 1/2 - 1/2 cos(2 pi (n + 1/2) / N)
    const float2* cs;               // (cos, sin)(pi j / n_theta), formed in double
    const float2* ph;               // (kappa n_theta)-th roots
    float2* Zr;                     // [pair][n_y][ncol]: the row transforms' bins k_x = column - cx - 1 (modulo 2 n_x)
    float2* M;                      // [pair][nrow][ncol]: (log1p |A|, log1p |B|) at k_y = row, k_x = column - cx - 1
    float2* Pr;                     // [pair][nrho][m_b]: F^B conj F^A of one radius, m = index + 1
};

static __global__ void k_roll_rows(RollParams p, AlignPairs q, int pair0)
{
    extern __shared__ float2 roll_lds[];
    const int y = blockIdx.x, pz = blockIdx.z, tid = threadIdx.x, T = blockDim.x, nx = p.nx, N = 2 * p.nx;
    float2* a = roll_lds;
    float2* b = a + lpad_size(N);
    const float wy = p.winY[y] / (float)(p.d * p.d);
    for (int x = tid; x < N; x += T)
        a[lpad(x)] = x < nx ? align_window_px(q.ref[pz], q.cur[pz], p.crop_x, p.crop_y, p.d, x, y, p.winX[x] * wy) : make_float2(0.0f, 0.0f);
    __syncthreads();
    const float2* r = fft_lds<-1, 1>(a, b, p.planX, p.twX, tid, T);
    float2* Z = p.Zr + ((long)(pair0 + pz) * p.ny + y) * p.ncol;
    for (int c = tid; c < p.ncol; c += T) Z[c] = r[lpad((c - p.cx - 1 + 2 * N) % N)];
}

static __global__ void k_roll_cols(RollParams p)
{
    extern __shared__ float2 roll_lds[];
    const int tid = threadIdx.x, T = blockDim.x, ny = p.ny, N = 2 * p.ny, pz = blockIdx.z;
    const int kx = blockIdx.x, c0 = p.cx + 1 + kx, c1 = p.cx + 1 - kx;      // the columns of k_x and -k_x; k_x = 0 is its own partner
    const bool same = kx == 0;
    float2* a = roll_lds;
    float2* b = a + lpad_size(2 * N);
    const float2* Z = p.Zr + (long)pz * ny * p.ncol;
    for (int g = tid; g < 2 * N; g += T) {
        const int y = g >> 1;
        a[lpad(g)] = y < ny ? Z[(long)y * p.ncol + ((g & 1) ? c1 : c0)] : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    const float2* f = fft_lds<-1, 2>(a, b, p.planY, p.twY, tid, T);
    float2* M = p.M + (long)pz * p.nrow * p.ncol;
    for (int g = tid; g < 2 * p.nrow; g += T) {
        const int col = g & 1, ky = g >> 1, kym = (N - ky) % N;
        if (same && col) continue;
        const float2 zk = f[lpad(g)], zm = f[lpad(2 * kym + (1 - col))];
        const float2 A = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
        const float2 B = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
        M[(long)ky * p.ncol + (col ? c1 : c0)] = make_float2(log1pf(hypotf(A.x, A.y)), log1pf(hypotf(B.x, B.y)));
    }
}

static __global__ void k_roll_polar(RollParams p)
{
    extern __shared__ float2 roll_lds[];
    const int tid = threadIdx.x, T = blockDim.x, nt = p.nt, pz = blockIdx.z;
    const float rho = (float)(p.rho_min + (int)blockIdx.x);
    float2* a = roll_lds;
    float2* b = a + lpad_size(2 * nt);
    const float2* M = p.M + (long)pz * p.nrow * p.ncol;
    for (int j = tid; j < nt; j += T) {
        const float2 cs = p.cs[j];
        const float kx = rho * cs.x * (float)p.sx, ky = rho * cs.y * (float)p.sy;
        const float x0 = floorf(kx), y0 = floorf(ky);
        const float fx = kx - x0, fy = ky - y0;
        // |k_x| <= cx and 0 <= k_y <= cy by the geometry (|cos|, sin <= 1 and rounding is monotone); the clamps keep a bad table in bounds
        const int ca = min(max((int)x0 + p.cx + 1, 0), p.ncol - 2), ra = min(max((int)y0, 0), p.nrow - 2);
        const float2* m0 = M + (long)ra * p.ncol + ca;
        const float2 m00 = m0[0], m01 = m0[1], m10 = m0[p.ncol], m11 = m0[p.ncol + 1];
        const float ta = m00.x + fx * (m01.x - m00.x), ba = m10.x + fx * (m11.x - m10.x);
        const float tb = m00.y + fx * (m01.y - m00.y), bb = m10.y + fx * (m11.y - m10.y);
        a[lpad(2 * j)] = make_float2(ta + fy * (ba - ta), 0.0f);
        a[lpad(2 * j + 1)] = make_float2(tb + fy * (bb - tb), 0.0f);
    }
    __syncthreads();
    const float2* f = fft_lds<-1, 2>(a, b, p.planT, p.twT, tid, T);
    float2* P = p.Pr + ((long)pz * p.nrho + blockIdx.x) * p.mb;
    for (int m = 1 + tid; m <= p.mb; m += T) {
        const float2 FA = f[lpad(2 * m)], FB = f[lpad(2 * m + 1)];
        P[m - 1] = make_float2(FB.x * FA.x + FB.y * FA.y, FB.y * FA.x - FB.x * FA.y);
    }
}

static __global__ void k_roll_peak(RollParams p, float* angles)
{
    extern __shared__ float2 roll_lds[];
    __shared__ float2 Rs[ROLL_MAX_MB];            // R[m], m = index + 1
    __shared__ float fv[ROLL_MAX_FINE];           // n_theta r on the fine grid
    __shared__ float sv[16];
    __shared__ int si[16];
    const int tid = threadIdx.x, T = blockDim.x, nt = p.nt, mb = p.mb, pz = blockIdx.z, kappa = p.kappa, nf = 2 * kappa + 1;
    float2* a = roll_lds;
    float2* b = a + lpad_size(nt);
    // P[m]: the radii in one fixed order; the band's largest magnitude
    const float2* Pr = p.Pr + (long)pz * p.nrho * mb;
    float top = -INFINITY;
    int at = 0x7fffffff;
    for (int m = tid; m < mb; m += T) {
        float2 s = make_float2(0.0f, 0.0f);
        for (int r = 0; r < p.nrho; r++) { const float2 v = Pr[(long)r * mb + m]; s.x += v.x; s.y += v.y; }
        Rs[m] = s;
        align_better(top, at, hypotf(s.x, s.y), m);
    }
    align_block_argmax(top, at, sv, si, tid, T);
    const float floor_p = 1e-9f * top;
    for (int x = tid; x < nt; x += T) a[lpad(x)] = make_float2(0.0f, 0.0f);
    __syncthreads();
    for (int m = tid; m < mb; m += T) {
        const float2 P = Rs[m];
        const float mag = hypotf(P.x, P.y);
        float2 R = make_float2(0.0f, 0.0f);
        if (top > 0.0f && mag > floor_p) R = make_float2(P.x / mag, P.y / mag);
        Rs[m] = R;
        a[lpad(m + 1)] = R;
        a[lpad(nt - m - 1)] = make_float2(R.x, -R.y);
    }
    __syncthreads();
    const float2* r = fft_lds<1, 1>(a, b, p.planT, p.twT, tid, T);
    float vc = -INFINITY;
    int pk = 0x7fffffff;
    for (int x = tid; x < nt; x += T) align_better(vc, pk, r[lpad(x)].x, x);
    align_block_argmax(vc, pk, sv, si, tid, T);
    // the fine grid: n_theta r(p + (i - kappa) / kappa) = 2 Re sum_{m = 1}^{m_b} R[m] exp(2 pi i m (p kappa + i - kappa) / (kappa n_theta))
    const int Mr = kappa * nt;
    for (int i = tid; i < nf; i += T) {
        int q = (pk * kappa + i - kappa) % Mr;
        if (q < 0) q += Mr;
        int idx = q;
        double acc = 0.0;
        for (int m = 0; m < mb; m++) {
            const float2 e = p.ph[idx], rr = Rs[m];
            acc += (double)rr.x * (double)e.x - (double)rr.y * (double)e.y;
            idx += q;
            if (idx >= Mr) idx -= Mr;
        }
        fv[i] = (float)(2.0 * acc);
    }
    __syncthreads();
    float v = -INFINITY;
    int best = 0x7fffffff;
    for (int i = tid; i < nf; i += T) align_better(v, best, fv[i], i);
    align_block_argmax(v, best, sv, si, tid, T);
    if (tid == 0) {
        float delta = 0.0f;
        if (best > 0 && best < nf - 1) {
            const float den = fv[best - 1] - 2.0f * v + fv[best + 1];
            if (den != 0.0f) delta = 0.5f * (fv[best - 1] - fv[best + 1]) / den;
        }
        float s = (float)pk + ((float)(best - kappa) + delta) / (float)kappa;
        s -= (float)nt * floorf((s + 0.5f * (float)nt) / (float)nt);
        const float K = (float)(2 * mb);
        const float4 res = make_float4(3.14159265358979323846f * s / (float)nt, v / K, vc / K, 0.0f);
        float* out = angles + 4 * (long)pz;
        if (((uintptr_t)out & 15) == 0) *(float4*)out = res;
        else { out[0] = res.x; out[1] = res.y; out[2] = res.z; out[3] = res.w; }
    }
}

}  // namespace fftup
