// rotate_phase_driver.cpp -- the phase arithmetic of csrc/rotate_phase.hpp (what the shear kernels run on the device) compiled with
// the host compiler, for tests/test_host_rotate.py: no device needed.
//   rotate_phase_driver N DELTA K [K ...]  ->  per bin K one line "K re im" with the fp32 values (ONE rounding of the double pair,
//   as the kernels round) as hex floats; DELTA is read as a hex or decimal double.
//   rotate_phase_driver coefficients THETA  ->  "a b" (%a): the shear coefficients of a rotation by THETA
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rotate_phase.hpp"

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "coefficients")) {
        const double t = strtod(argv[2], nullptr);
        printf("%a %a\n", fftup_rotphase::shear_a(t), fftup_rotphase::shear_b(t));
        return 0;
    }
    if (argc < 4) return 2;
    const int n = atoi(argv[1]);
    const double delta = strtod(argv[2], nullptr);
    if (n < 2) return 2;
    std::vector<float> out;
    for (int i = 3; i < argc; i++) {
        const int k = atoi(argv[i]);
        if (k < 0 || k >= n) return 2;
        const fftup_rotphase::Cplx w = fftup_rotphase::shear_factor(k, n, delta);
        out.push_back((float)w.re);
        out.push_back((float)w.im);
        printf("%d %a %a\n", k, (double)out[out.size() - 2], (double)out[out.size() - 1]);
    }
    return 0;
}
