// Prints the host tables of one axis of a mirror view plan (csrc/mirror_tables.hpp) for tests/test_host_mirror.py: no device needed.
//   mirror_tables_driver N M origin span  ->  "kmax L ncols", then the pre, post and bhat tables, one "re im" pair per line (%.9g: exact fp32)
#include <cstdio>
#include <cstdlib>

#include "mirror_tables.hpp"

int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const uint32_t N = (uint32_t)strtoul(argv[1], nullptr, 10), M = (uint32_t)strtoul(argv[2], nullptr, 10);
    const double origin = strtod(argv[3], nullptr), span = strtod(argv[4], nullptr);
    const uint32_t L = fftup_viewtab::mirror_conv_length(N, M);
    fftup_viewtab::AxisTables t;
    fftup_viewtab::make_mirror_axis(N, M, origin, span, L, t);
    printf("%d %u %d\n", t.kmax, L, fftup_viewtab::mirror_ncols(N, t.kmax));
    for (const std::vector<float>* v : {&t.pre, &t.post, &t.bhat})
        for (size_t i = 0; i < v->size(); i += 2) printf("%.9g %.9g\n", (double)(*v)[i], (double)(*v)[i + 1]);
    return 0;
}
