// mirror_tables.hpp -- the host side of view plans with FFTUP_FLAG_MIRROR (include/fftup.h, kernels_mirror.hpp).  Plain C++ (no
// HIP), beside view_tables.hpp: tests/mirror/mirror_tables_driver.cpp prints the tables for tests/test_host_mirror.py.
//
// One axis N -> M with the view (origin, span): the frame's half-sample even reflection has period 2N and the spectrum
// X~[f] = 2 exp(i pi f / 2N) C[|f|] (C: the DCT-II of the N samples, C[N] = 0).  Its view is view_tables.hpp's axis of period 2N
// aimed at origin + 1/2: pre[j] then carries exp(i pi f (2 origin + 1) / 2N) -- the phase of X~ included -- the weight g = 1/2 of
// |f| = N lands on the zero bin, post carries 1/(2N) (span/M), and the kernels put in Z_f = 2 C[|f|].  The phases are twice as
// long as a periodic view's: the same long double reduction, origin + 1/2 formed in long double (exact).
#pragma once
#include "view_tables.hpp"

namespace fftup_viewtab {

// the convolution length: that of the doubled period, the smallest 2,3,5,7-smooth L >= 2N + M (kmax = N: 2N + 1 bins in)
inline uint32_t mirror_conv_length(uint32_t N, uint32_t M) { return conv_length(2 * N, M); }

// the last cosine a view reaches: min(N, floor(N M / max(span, M))) -- N itself only as the zero bin
inline int mirror_kmax_of(uint32_t N, uint32_t M, double span) { return kmax_of(2 * N, M, span); }

// bins of the reordered rows' half spectrum the frame needs: C[k] comes from bin k for 2k <= N and from bin N - k above
inline int mirror_ncols(uint32_t N, int kmax) { return kmax < (int)(N / 2) ? kmax + 1 : (int)(N / 2) + 1; }

// t.kmax may be N (K = 2N + 1 entries of pre); chirp as make_axis
inline void make_mirror_axis(uint32_t N, uint32_t M, double origin, double span, uint32_t L, AxisTables& t, bool chirp = true)
{
    make_axis(2 * N, M, (long double)origin + 0.5L, span, L, t, chirp);
}

}  // namespace fftup_viewtab
