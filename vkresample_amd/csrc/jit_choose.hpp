// jit_choose.hpp / jit_choose.cpp -- the plan-time chooser: which factorizations a plan specialised at plan time runs
// (jit.hpp has the whole picture).  Measured rules, a built-in table of tuner results for the MI355X and the user's wisdom
// file; arithmetic and one text file, no device and no compiler (plan_rules.hpp and the device-free drivers of tests/ need
// nothing else of the plan-time compiler).
#pragma once
#include <cstddef>
#include <string>
#include <vector>

namespace fftup_jit {

struct Choice {
    int W = 0, H = 0, UW = 0;
    int U = 2;                         // integer upscale factor; 1 = half-integer factor D/2 (one spectrum buffer with all rows)
    int D = 4;                         // 2 DD x upscale factor: the spectrum rows hold kx = 0..UW DD / D
    int DD = 1;                        // 1: integer and half-integer factors (D = 2u); 2: quarter-integer ones (D = 4u, odd: -u 1.25 -> 5)
    int UH = 0;
    bool half = false;
    int row_kind = -1;                 // 0: k_row_r2c_t<W> (power of two, 8 points per thread); 1: k_row_r2c_m (three stages); 2: k_row_r2c (not specialised); 3: k_row_r2c_n
    int rr[3] = {0, 0, 0}, row_t = 0;
    std::vector<int> rn, cn;           // kind 3: k_row_r2c_n / k_col_n (N stages)
    std::vector<int> ci;               // col kind 5: the inverse transform of length UH
    int col_cols = 4;                  // col kinds 3-5: columns of a 4-wide spectrum tile per workgroup (4, or 2 for long columns)
    int col_kind = -1;                 // 0: k_col_t<H>; 1: k_col_m (three stages); 3: k_col_n (N stages); 4: k_col_u (N stages, U - 1 residues); 5: k_col_pad (half-integer factors)
    int cr[3] = {0, 0, 0}, col_tpc = 0;
    int fused_kind = -1;               // 0: FusedPlanPow2<UW>; 1: FusedPlanMr16<UW, UW/256>; 2: FusedPlanN<UW, T, 2, radices...>
    std::vector<int> fr;
    int fused_t = 0;
    int fused_wpe = 0;                 // kind 2: waves per SIMD the fused kernel's register allocation must allow
    bool fused_rr = true;              // kind 2: ring rows in registers
    std::vector<int> ct;               // stand-alone C2R (pre-sharpen tap): CtPlan<UW, ct_t, radices...>
    int ct_t = 0;
    // launch geometry derived from the above (what the device-side templates compute for themselves)
    int row_block = 0, col_block = 0;
    size_t col_lds = 0, fused_lds = 0, ct_lds = 0;
    bool u8out = false;                // fused kernel stores interleaved 8-bit RGB (FFTUP_FLAG_FUSE_U8_STORE)
};

// Test knobs: FFTUP_EXPERIMENT="key=value;key=value" pins factorizations and strip lengths for tests and tools (keys: aot,
// g_per_cu, pairs_per_strip, jit_tune, jit_row, jit_col, jit_coli, jit_fused, jit_fused_opt, jit_row_nstage, jit_col_nstage,
// jit_no_builtin_wisdom, jit_dump, jit_threads).  The parser exists only in a library built with -DFFTUP_TEST_KNOBS
// (libfftup_knobs.so, which the tests that pin something load; it lives in jit.cpp, the one unit compiled twice); in the
// shipping library this returns nullptr, whatever the environment says.  Returns the value ("" for a bare key) or nullptr.
const char* experiment(const char* key);

struct FusedCand { int T; std::vector<int> r; };

// factorizations for a W x H plan with upscale factor D/2 (radices of the stand-alone C2R given); `arch`: the wisdom key's
// device part ("" = none); false: no specialised factorization exists
bool choose(int W, int H, int D, bool half, const std::vector<int>& ct_radices, Choice& c, const std::string& arch = "", bool use_wisdom = true, int DD = 1);
std::string describe(const Choice& c);
// alternatives for the fused kernel of a row length (the tuner's candidates), the chooser's pick first
std::vector<FusedCand> fused_candidates(int n, int D, size_t max, int DD = 1);
void set_fused_n(Choice& c, int T, const std::vector<int>& radices);
std::string fused_key(const Choice& c, const std::string& arch);
std::string fused_value(const Choice& c);
bool wisdom_lookup(const std::string& key, std::string& value);
void wisdom_store(const std::string& key, const std::string& value);

// ---- internal: shared by jit_choose.cpp (the wisdom file) and jit.cpp (code objects, kernel headers)
std::string cache_dir();               // $FFTUP_CACHE_DIR, else $XDG_CACHE_HOME/fftup, else ~/.cache/fftup, created; "" = none
bool read_file(const std::string& path, std::string& out);
std::string join(const std::vector<int>& v);       // "r0, r1, .."

}  // namespace fftup_jit
