// jit_choose_driver.cpp -- the plan-time chooser (csrc/jit.hpp: choose, describe, fused_candidates) without a device or a
// compiler.  One request per line on standard input, one answer line each:
//   choose W H D DD half use_wisdom ARCHKEY   every field of the Choice, or "none" (ARCHKEY "-" = the empty key)
//   cands N D DD MAX                          the tuner's candidates, "T:r0,r1,.." in order
// A choose line has four parts, joined by " | ": row, column, fused kernel, stand-alone C2R, each with the sizes it depends
// on; the first three carry their share of describe()'s text.  fused_key, fused_value and set_fused_n are exercised on the
// way (printed with the fused part).  Linked with the library's object files (tests/jit_choose_lib.py); the environment
// (FFTUP_CACHE_DIR with a wisdom.txt, FFTUP_EXPERIMENT for the build with the test knobs) is the caller's.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "jit.hpp"

static std::string list(const std::vector<int>& v)
{
    std::string s;
    for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
    return s.empty() ? "-" : s;
}
static std::string list(const int (&v)[3]) { return list(std::vector<int>(v, v + 3)); }

// the stage list of a stand-alone C2R (radices <= 8): what a caller hands to choose(), which only copies it
static std::vector<int> ct_radices(int n)
{
    std::vector<int> r;
    for (int q : {8, 7, 5, 4, 3, 2})
        while (n % q == 0) { r.push_back(q); n /= q; }
    return r;
}

static void print_choice(const fftup_jit::Choice& c, const std::string& arch)
{
    // describe(): "<factor> row <row>, col <col>, fused <fused>"
    const std::string d = fftup_jit::describe(c);
    const size_t a = d.find("row "), b = d.find(", col "), f = d.find(", fused ");
    if (a == std::string::npos || b == std::string::npos || f == std::string::npos) { printf("bad description: %s\n", d.c_str()); return; }
    printf("row W=%d kind=%d rr=%s t=%d rn=%s block=%d text=[%s]", c.W, c.row_kind, list(c.rr).c_str(), c.row_t, list(c.rn).c_str(), c.row_block,
           d.substr(a, b - a).c_str());
    printf(" | col H=%d UH=%d U=%d kind=%d cr=%s tpc=%d cn=%s ci=%s cols=%d block=%d lds=%zu text=[%s]", c.H, c.UH, c.U, c.col_kind, list(c.cr).c_str(),
           c.col_tpc, list(c.cn).c_str(), list(c.ci).c_str(), c.col_cols, c.col_block, c.col_lds, d.substr(b + 2, f - b - 2).c_str());
    printf(" | fused UW=%d D=%d DD=%d half=%d u8out=%d kind=%d fr=%s t=%d wpe=%d rr=%d lds=%zu key=[%s] value=[%s] text=[%s%s]", c.UW, c.D, c.DD,
           (int)c.half, (int)c.u8out, c.fused_kind, list(c.fr).c_str(), c.fused_t, c.fused_wpe, (int)c.fused_rr, c.fused_lds, fftup_jit::fused_key(c, arch).c_str(),
           fftup_jit::fused_value(c).c_str(), d.substr(0, a).c_str(), d.substr(f + 2).c_str());
    if (c.fused_kind == 2) {           // set_fused_n on a copy: the geometry a tuner candidate with these radices gets
        fftup_jit::Choice t = c;
        fftup_jit::set_fused_n(t, c.fused_t, c.fr);
        printf(" set=%d,%d,%zu", t.fused_wpe, (int)t.fused_rr, t.fused_lds);
    }
    printf(" | ct r=%s t=%d lds=%zu\n", list(c.ct).c_str(), c.ct_t, c.ct_lds);
}

int main()
{
    std::string line, word;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> word;
        if (word == "choose") {
            int W, H, D, DD, half, use_wisdom;
            std::string arch;
            in >> W >> H >> D >> DD >> half >> use_wisdom >> arch;
            if (!in) { fprintf(stderr, "bad request line: %s\n", line.c_str()); return 2; }
            if (arch == "-") arch.clear();
            fftup_jit::Choice c;
            if (!fftup_jit::choose(W, H, D, half != 0, ct_radices(D * W / (2 * DD)), c, arch, use_wisdom != 0, DD)) { printf("none\n"); continue; }
            print_choice(c, arch);
        } else if (word == "cands") {
            int n, D, DD;
            size_t max;
            in >> n >> D >> DD >> max;
            if (!in) { fprintf(stderr, "bad request line: %s\n", line.c_str()); return 2; }
            std::string s;
            for (const auto& cand : fftup_jit::fused_candidates(n, D, max, DD)) s += (s.empty() ? "" : " ") + std::to_string(cand.T) + ":" + list(cand.r);
            printf("%s\n", s.empty() ? "-" : s.c_str());
        } else { fprintf(stderr, "bad request line: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
