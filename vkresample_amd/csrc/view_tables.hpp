// view_tables.hpp -- the host side of the view plans (fftup_plan_create_view, include/fftup.h): per axis, how many bins a view keeps,
// the length of its cyclic convolution and the three chirp tables of kernels_view.hpp.  Plain C++ (no HIP): the planner includes
// it, and tests/view/view_tables_driver.cpp prints the tables for tests/test_host_view.py without a device.
//
// One axis N -> M with the view (origin, span), step s = span / M, theta = 2 pi / N, K = 2 kmax + 1 bins at j = f + kmax:
//     y[m] = post[m] * sum_j (Z_j pre[j]) c[m - j]
//     pre[j]  = g exp(i theta ((j - kmax) origin + s j^2 / 2)),    g = 1/2 where 2 |j - kmax| == N, else 1
//     post[m] = norm exp(i theta (s m^2 / 2 - kmax m s)),          norm = (1/N) (span/M)
//     c[d]    = exp(-i theta s d^2 / 2),  d in [-(K - 1), M - 1];  bhat = FFT_L(c wrapped) / L
// The phases are formed in long double in units of pi (x = 2 (j - kmax) origin / N + s j^2 / N ...), reduced with fmodl(x, 2) BEFORE
// the multiplication by pi -- they reach tens of thousands of radians -- and rounded once to fp32.  origin is reduced modulo N first.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <vector>

namespace fftup_viewtab {

inline bool smooth(uint32_t n)
{
    if (n == 0) return false;
    for (uint32_t p : {2u, 3u, 5u, 7u})
        while (n % p == 0) n /= p;
    return n == 1;
}

// the convolution length of an axis: the smallest 2,3,5,7-smooth L >= (2 (N/2) + 1) + M - 1 -- the worst case kmax = N/2, so
// every view of the same N and M fits
inline uint32_t conv_length(uint32_t N, uint32_t M)
{
    uint32_t L = 2 * (N / 2) + M;
    while (!smooth(L)) L++;
    return L;
}

// the last bin a view keeps, in double exactly as include/fftup.h writes it: N M is exact, the quotient correctly rounded
inline int kmax_of(uint32_t N, uint32_t M, double span)
{
    const double q = std::floor((double)((uint64_t)N * (uint64_t)M) / (2.0 * std::max(span, (double)M)));
    return (int)std::min((double)(N / 2), q);
}

// DFT with exp(+2 pi i nk / n) of a smooth length in double (recursive decimation in time by the smallest prime factor)
inline void host_fft(std::vector<std::complex<double>>& x)
{
    const size_t n = x.size();
    if (n <= 1) return;
    size_t p = 2;
    while (n % p) p++;
    const size_t m = n / p;
    std::vector<std::vector<std::complex<double>>> sub(p, std::vector<std::complex<double>>(m));
    for (size_t j = 0; j < m; j++)
        for (size_t r = 0; r < p; r++) sub[r][j] = x[j * p + r];
    for (auto& v : sub) host_fft(v);
    for (size_t k = 0; k < n; k++) {
        std::complex<double> acc = sub[0][k % m];
        for (size_t r = 1; r < p; r++) acc += sub[r][k % m] * std::polar(1.0, 2.0 * M_PI * (double)((r * k) % n) / (double)n);
        x[k] = acc;
    }
}

struct AxisTables {
    int kmax = 0;
    std::vector<float> pre, post, bhat;      // interleaved (re, im): 2 kmax + 1, M and L points
};

// exp(i pi x) in long double, x reduced modulo 2 first
inline std::complex<long double> expipi(long double x)
{
    const long double r = fmodl(x, 2.0L), a = 3.141592653589793238462643383279502884L * r;
    return std::complex<long double>(cosl(a), sinl(a));
}

// chirp = false: only `pre` (the one table the origin enters) is rebuilt -- a pan at an unchanged span
// (origin: a double, or -- mirror_tables.hpp -- a double plus one half, exact in long double)
inline void make_axis(uint32_t N, uint32_t M, long double origin, double span, uint32_t L, AxisTables& t, bool chirp = true)
{
    const int kmax = kmax_of(N, M, span), K = 2 * kmax + 1;
    const long double n = (long double)N, s = (long double)span / (long double)M, o = fmodl(origin, n);
    t.kmax = kmax;
    t.pre.resize(2 * (size_t)K);
    for (int j = 0; j < K; j++) {
        const long double f = (long double)(j - kmax), jj = (long double)j;
        const long double g = 2 * (uint32_t)std::abs(j - kmax) == N ? 0.5L : 1.0L;
        const std::complex<long double> w = expipi(fmodl(2.0L * f * o / n, 2.0L) + fmodl(s * jj * jj / n, 2.0L));
        t.pre[2 * j] = (float)(g * w.real()); t.pre[2 * j + 1] = (float)(g * w.imag());
    }
    if (!chirp) return;
    t.post.resize(2 * (size_t)M); t.bhat.resize(2 * (size_t)L);
    const long double norm = (1.0L / n) * s;
    for (uint32_t m = 0; m < M; m++) {
        const long double mm = (long double)m;
        const std::complex<long double> w = expipi(fmodl(s * mm * mm / n, 2.0L) - fmodl(2.0L * (long double)kmax * mm * s / n, 2.0L));
        t.post[2 * m] = (float)(norm * w.real()); t.post[2 * m + 1] = (float)(norm * w.imag());
    }
    std::vector<std::complex<double>> c(L, std::complex<double>(0.0, 0.0));
    for (int d = -(K - 1); d <= (int)M - 1; d++) {       // (K + M - 1 <= L: the two wings do not meet)
        const long double dd = (long double)d;
        const std::complex<long double> w = expipi(-fmodl(s * dd * dd / n, 2.0L));
        c[(size_t)(d < 0 ? d + (int)L : d)] = std::complex<double>((double)w.real(), (double)w.imag());
    }
    host_fft(c);
    for (uint32_t k = 0; k < L; k++) {
        t.bhat[2 * k] = (float)(c[k].real() / (double)L); t.bhat[2 * k + 1] = (float)(c[k].imag() / (double)L);
    }
}

}  // namespace fftup_viewtab
