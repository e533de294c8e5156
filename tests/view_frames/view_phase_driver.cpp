// Holds the fp64 phase arithmetic of csrc/view_phase.hpp (what k_view_tables runs on the device) to the long double host tables of
// csrc/view_tables.hpp / mirror_tables.hpp, for tests/test_host_view_frames.py: no device needed.
//   view_phase_driver N M origin span mirror  ->  "kmax L", then per table (pre, post, bhat) one line
//   "<name> <max |difference|> <max |table|> <their quotient>" (%.9g).  bhat: host_fft of the fp64 chirp, / L, rounded once.
#include <cstdio>
#include <cstdlib>

#include "mirror_tables.hpp"
#include "view_phase.hpp"
#include "view_tables.hpp"

static void report(const char* name, const std::vector<float>& got, const std::vector<float>& want)
{
    double diff = 0, top = 0;
    if (got.size() != want.size()) { printf("%s size mismatch\n", name); exit(3); }
    for (size_t i = 0; i < got.size(); i++) {
        diff = std::max(diff, std::fabs((double)got[i] - (double)want[i]));
        top = std::max(top, std::fabs((double)want[i]));
    }
    printf("%s %.9g %.9g %.9g\n", name, diff, top, top > 0 ? diff / top : diff);
}

int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const uint32_t N = (uint32_t)strtoul(argv[1], nullptr, 10), M = (uint32_t)strtoul(argv[2], nullptr, 10);
    const double origin = strtod(argv[3], nullptr), span = strtod(argv[4], nullptr);
    const bool mirror = atoi(argv[5]) != 0;
    const uint32_t L = mirror ? fftup_viewtab::mirror_conv_length(N, M) : fftup_viewtab::conv_length(N, M);
    fftup_viewtab::AxisTables t;
    if (mirror) fftup_viewtab::make_mirror_axis(N, M, origin, span, L, t);
    else fftup_viewtab::make_axis(N, M, origin, span, L, t);

    const int kmax = mirror ? fftup_viewtab::mirror_kmax_of(N, M, span) : fftup_viewtab::kmax_of(N, M, span), K = 2 * kmax + 1;
    if (kmax != t.kmax) { printf("kmax mismatch\n"); return 3; }
    const uint32_t n = mirror ? 2 * N : N;
    const fftup_viewphase::Axis a = fftup_viewphase::axis_of(n, M, fftup_viewphase::origin_of(origin, (double)n, mirror), span, kmax);
    std::vector<float> pre(2 * (size_t)K), post(2 * (size_t)M), bhat(2 * (size_t)L);
    for (int j = 0; j < K; j++) {
        const fftup_viewphase::Cplx w = fftup_viewphase::pre_of(a, j);
        pre[2 * j] = (float)w.re; pre[2 * j + 1] = (float)w.im;
    }
    for (uint32_t m = 0; m < M; m++) {
        const fftup_viewphase::Cplx w = fftup_viewphase::post_of(a, (int)m);
        post[2 * m] = (float)w.re; post[2 * m + 1] = (float)w.im;
    }
    std::vector<std::complex<double>> c(L);
    for (uint32_t i = 0; i < L; i++) {
        const fftup_viewphase::Cplx w = fftup_viewphase::chirp_wrapped(a, (int)i, (int)L);
        c[i] = std::complex<double>(w.re, w.im);
    }
    fftup_viewtab::host_fft(c);
    for (uint32_t k = 0; k < L; k++) {
        bhat[2 * k] = (float)(c[k].real() / (double)L); bhat[2 * k + 1] = (float)(c[k].imag() / (double)L);
    }
    printf("%d %u\n", kmax, L);
    report("pre", pre, t.pre);
    report("post", post, t.post);
    report("bhat", bhat, t.bhat);
    return 0;
}
