// shift_path_driver -- csrc/shift_path.hpp on the CPU: the functions k_shift_path runs, driven serially.
// stdin:  mode sigma min_peak n, then n rows of four fp32 bit patterns in hex (dx dy peak peak_coarse)
// stdout: n lines "p_x p_y s_x s_y out_x out_y" with %.17g (out: rounded to fp32 as fftup_shift_path stores it)
// The scan is BLOCKED the way the kernel's is -- four frames per block, the blocks' totals joined in order -- so that the operator's
// associativity is exercised, not only its serial use.  Test infrastructure only.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "shift_path.hpp"

namespace sp = fftup_shiftpath;

static float bits(uint32_t u)
{
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

int main()
{
    unsigned mode = 0, n = 0;
    float sigma_f = 0, min_peak = 0;
    if (scanf("%u %f %f %u", &mode, &sigma_f, &min_peak, &n) != 4 || mode > 1 || n == 0 || n > sp::MAX_FRAMES) return 2;
    std::vector<sp::Elem> e(n);
    for (unsigned i = 0; i < n; i++) {
        uint32_t u[4];
        if (scanf("%x %x %x %x", &u[0], &u[1], &u[2], &u[3]) != 4) return 2;
        e[i] = sp::elem_of(mode, i, bits(u[0]), bits(u[1]), bits(u[2]), min_peak);
    }
    // blocks of four scanned serially, the blocks' totals scanned, then joined in front of each block's frames
    const unsigned B = 4, nb = (n + B - 1) / B;
    std::vector<sp::Elem> total(nb);
    for (unsigned b = 0; b < nb; b++) {
        sp::Elem run{0, 0.0, 0.0};
        for (unsigned i = b * B; i < n && i < (b + 1) * B; i++) { run = sp::join(run, e[i]); e[i] = run; }
        total[b] = run;
    }
    sp::Elem base{0, 0.0, 0.0};
    for (unsigned b = 0; b < nb; b++) {
        for (unsigned i = b * B; i < n && i < (b + 1) * B; i++) e[i] = sp::join(base, e[i]);
        base = sp::join(base, total[b]);
    }
    const double sigma = (double)sigma_f;
    const int r = sp::radius_of(sigma);
    std::vector<double> g((size_t)r + 1, 1.0);
    for (int j = 0; r && j <= r; j++) g[(size_t)j] = sp::weight_of(j, sigma);
    const auto weight = [&](int j) { return g[(size_t)j]; };
    for (unsigned i = 0; i < n; i++) {
        double sx = 0.0, sy = 0.0;
        if (r) {
            sx = sp::smoothed_at([&](int k) { return e[(size_t)k].x; }, weight, (int)i, (int)n, r);
            sy = sp::smoothed_at([&](int k) { return e[(size_t)k].y; }, weight, (int)i, (int)n, r);
        }
        printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", e[i].x, e[i].y, sx, sy, (double)(float)(e[i].x - sx), (double)(float)(e[i].y - sy));
    }
    return 0;
}
