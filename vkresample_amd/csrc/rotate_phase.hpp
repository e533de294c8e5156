// rotate_phase.hpp -- the phase factors of a shear pass (include/fftup.h, "rotation by three shears"), for the host and for the
// device alike: k_rotate_shear_x / k_rotate_shear_y (kernels_rotate.hpp) multiply the bins of a row or column with these
// functions, tests/rotate/rotate_phase_driver.cpp holds them to numpy in extended precision on the CPU.  Plain C++ with
// __host__ __device__ functions when compiled as HIP; no HIP calls, no long double.
//
// A line of n points moved by delta pixels: bin k (signed f = k for 2 k < n, k - n for 2 k > n) is multiplied by
//     exp(-2 pi i f delta / n),        and for even n the Nyquist bin k = n / 2 by the real  cos(pi delta).
// f delta / n reaches a thousand turns (delta up to 2048 pixels, f up to 2048): in fp32 nothing of the phase would be left.  So
// t = f delta / n is formed in double (f delta: one rounding, the quotient: another -- 2e-13 turns at a thousand turns), reduced to
// r = t - rint(t) in [-1/2, 1/2] (exact), and only then handed to sincospi; delta is reduced modulo 2 (exactly: fmod-like by
// rint of delta / 2) before cospi.  The caller rounds ONCE to fp32.  delta = 0 gives exactly (1, 0) for every bin.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FFTUP_ROTPHASE_HD __host__ __device__
#else
#define FFTUP_ROTPHASE_HD
#endif

namespace fftup_rotphase {

struct Cplx { double re, im; };

// the two shear coefficients of a rotation by theta: x-shears by a = -tan(theta / 2), the y-shear by b = sin(theta)
inline double shear_a(double theta) { return -std::tan(0.5 * theta); }
inline double shear_b(double theta) { return std::sin(theta); }

// exp(i pi x) for |x| <= 1: exact at the multiples of 1/2
FFTUP_ROTPHASE_HD inline Cplx expipi(double x)
{
    Cplx w;
#if defined(__HIP_DEVICE_COMPILE__)
    ::sincospi(x, &w.im, &w.re);
#else
    // the quadrant first (q = rint(2 x), y = x - q / 2 in [-1/4, 1/4], both exact), so that the zeros come out as zeros
    const double q = std::rint(2.0 * x), y = x - 0.5 * q, ang = 3.14159265358979323846 * y;
    const double s = std::sin(ang), c = std::cos(ang);
    switch ((int)q & 3) {            // (two's complement: -1 & 3 == 3)
    case 0: w.re = c; w.im = s; break;
    case 1: w.re = -s; w.im = c; break;
    case 2: w.re = -c; w.im = -s; break;
    default: w.re = s; w.im = -c; break;
    }
#endif
    return w;
}

// the factor of bin k of a line of n points moved by delta
FFTUP_ROTPHASE_HD inline Cplx shear_factor(int k, int n, double delta)
{
    if (2 * k == n) {                                    // the Nyquist bin of an even length: real
        const double d = delta - 2.0 * std::rint(0.5 * delta);      // delta modulo 2, in [-1, 1]
        return {expipi(d).re, 0.0};
    }
    const int f = 2 * k < n ? k : k - n;
    const double t = (double)f * delta / (double)n;
    const double r = t - std::rint(t);              // in [-1/2, 1/2], exact
    return expipi(-2.0 * r);
}

}  // namespace fftup_rotphase
