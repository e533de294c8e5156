// view_phase.hpp -- the three chirp tables of a view axis (view_tables.hpp: pre, post, the chirp c) restated in fp64, for the host
// and for the device alike: k_view_tables (kernels_view_tables.hpp) builds the tables of fftup_execute_device_views with these
// functions, tests/view_frames/view_phase_driver.cpp holds them to make_axis / make_mirror_axis on the CPU.  Plain C++ with
// __host__ __device__ functions when compiled as HIP; no HIP calls, no long double.
//
// One axis n -> M (n: the period -- N, or 2N of a mirror axis), step s = span / M, K = 2 kmax + 1 bins at j = f + kmax:
//     pre[j]  = g exp(i pi (2 f o / n + s j^2 / n)),          g = 1/2 where 2 |f| == n, else 1;  o = origin (+ 1/2: mirror) mod n
//     post[m] = (1/n) s exp(i pi s m (m - 2 kmax) / n)
//     c[d]    = exp(-i pi s d^2 / n),  d in [-(K - 1), M - 1]
// Every phase is a quotient a q / n in units of pi with q an exact integer (2 f, j^2, m (m - 2 kmax), d^2 -- below 2^53) and `a` a
// real number carried as a pair of doubles (s, or o).  They reach 1e8 half-turns, where the plain a * q / n has lost eight of its
// sixteen digits before the reduction; so the product is formed exactly (fma two-product), divided with an fma remainder, the high
// quotient reduced modulo 2 by fmod (exact) and the low part added afterwards: the reduced phase is good to a few 1e-16
// half-turns whatever its size.  Then one multiplication by pi, one sin / cos and ONE rounding to fp32 by the caller.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FFTUP_PHASE_HD __host__ __device__
#else
#define FFTUP_PHASE_HD
#endif

namespace fftup_viewphase {

struct Pair { double hi, lo; };      // the real number hi + lo, |lo| <= ulp(hi) / 2

// span / M as a pair: the quotient and what the division left over
FFTUP_PHASE_HD inline Pair step_of(double span, double M)
{
    const double hi = span / M;
    return {hi, std::fma(-hi, M, span) / M};
}

// origin modulo n (fmod is exact), for a mirror axis + 1/2 (two-sum: exact as a pair)
FFTUP_PHASE_HD inline Pair origin_of(double origin, double n, bool mirror)
{
    const double o = std::fmod(origin, n);
    if (!mirror) return {o, 0.0};
    const double hi = o + 0.5, b = hi - o;
    return {hi, (o - (hi - b)) + (0.5 - b)};
}

// (a q / n) modulo 2 in (-2, 2) + a low part: q an exact integer in a double, n > 0
FFTUP_PHASE_HD inline double phase_mod2(Pair a, double q, double n)
{
    const double p_hi = a.hi * q;
    const double p_lo = std::fma(a.hi, q, -p_hi) + a.lo * q;        // a q = p_hi + p_lo
    const double t_hi = p_hi / n;
    const double rem = std::fma(-t_hi, n, p_hi);                    // exact: p_hi = t_hi n + rem
    const double t_lo = (rem + p_lo) / n;
    return std::fmod(t_hi, 2.0) + t_lo;
}

struct Cplx { double re, im; };

// exp(i pi x), x reduced modulo 2 first
FFTUP_PHASE_HD inline Cplx expipi(double x)
{
    const double r = std::fmod(x, 2.0);
    Cplx w;
#if defined(__HIP_DEVICE_COMPILE__)
    ::sincospi(r, &w.im, &w.re);
#else
    const double a = 3.14159265358979323846 * r;
    w.re = std::cos(a); w.im = std::sin(a);
#endif
    return w;
}

// one axis: what the three formulas share.  n: the period -- the input length, doubled for a mirror axis; o = origin_of(origin, n, mirror)
struct Axis {
    double n, M;
    int kmax;
    Pair s, o;
    double norm;                     // (1/n) s, the magnitude of post
};
FFTUP_PHASE_HD inline Axis axis_of(uint32_t n, uint32_t M, Pair o, double span, int kmax)
{
    Axis a;
    a.n = (double)n; a.M = (double)M; a.kmax = kmax;
    a.s = step_of(span, a.M); a.o = o;
    a.norm = a.s.hi / a.n;
    return a;
}

// pre[j], j < 2 kmax + 1 (the weight g included)
FFTUP_PHASE_HD inline Cplx pre_of(const Axis& a, int j)
{
    const int f = j - a.kmax;
    const double jj = (double)j, g = 2.0 * (double)(f < 0 ? -f : f) == a.n ? 0.5 : 1.0;
    const Cplx w = expipi(phase_mod2(a.o, 2.0 * (double)f, a.n) + phase_mod2(a.s, jj * jj, a.n));
    return {g * w.re, g * w.im};
}

// post[m], m < M (the normalisation included)
FFTUP_PHASE_HD inline Cplx post_of(const Axis& a, int m)
{
    const double mm = (double)m;
    const Cplx w = expipi(phase_mod2(a.s, mm * (mm - 2.0 * (double)a.kmax), a.n));
    return {a.norm * w.re, a.norm * w.im};
}

// c[d], d in [-(K - 1), M - 1]
FFTUP_PHASE_HD inline Cplx chirp_of(const Axis& a, int d)
{
    const double dd = (double)d;
    return expipi(-phase_mod2(a.s, dd * dd, a.n));
}

// c wrapped to L points: c[i] for i < M, c[i - L] for i > L - K, zero between (K + M - 1 <= L: the two wings do not meet)
FFTUP_PHASE_HD inline Cplx chirp_wrapped(const Axis& a, int i, int L)
{
    if (i < (int)a.M) return chirp_of(a, i);
    if (i > L - (2 * a.kmax + 1)) return chirp_of(a, i - L);
    return {0.0, 0.0};
}

}  // namespace fftup_viewphase
