// jit_choose.cpp -- the plan-time chooser (see jit_choose.hpp)
#include "jit_choose.hpp"

#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace fftup_jit {

// radices the register engines have butterflies for (fft_engine.hpp bfly<R>, kernels_pow2.hpp twiddle_all<R>)
static const int kRadices[] = {2, 3, 4, 5, 7, 8, 9, 10, 12, 14, 15, 16};
static constexpr size_t kComplex = 8;              // bytes of a float2
static constexpr size_t kLdsMax = 160 * 1024;

static bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
static bool is_radix(int r) { for (int s : kRadices) if (s == r) return true; return false; }
static int round_up(int x, int granule) { return (x + granule - 1) / granule * granule; }

// depth-first over the ordered factorizations of m into at most `depth` radices, radices ascending.  The order is part of
// every choice below: all their comparisons are strict, so the first factorization found wins a tie.
template <class Visit>
static void each_factorization(int m, size_t depth, std::vector<int>& cur, const Visit& visit)
{
    if (m == 1) { visit(cur); return; }
    if (cur.size() >= depth) return;
    for (int r : kRadices)
        if (m % r == 0) { cur.push_back(r); each_factorization(m / r, depth, cur, visit); cur.pop_back(); }
}

// Every stage moves all n points through LDS once and multiplies them by twiddles, whatever its radix, so the work of a
// factorization is decided by its NUMBER of stages; between factorizations with equally many stages the lane slots
// count (threads x points per thread, idle lanes included): balanced radices need the fewest threads.
struct StageCost { int points, min_radix; double slots; };          // most points a thread holds in a stage; smallest radix; lane slots
static StageCost stage_cost(int n, const std::vector<int>& r, int T)
{
    StageCost c = {0, 99, 0};
    for (int q : r) {
        const int bpt = (n / q + T - 1) / T;                         // butterflies per thread
        c.points = std::max(c.points, bpt * q);
        c.min_radix = std::min(c.min_radix, q);
        c.slots += (double)bpt * T * q;
    }
    return c;
}

// "T:r0,r1,.." or "r0,r1,.." (T = 0): a pinned factorization (experiment keys) or a wisdom value
static bool parse_radices(const char* text, std::vector<int>& r, int& T)
{
    std::string s = text;
    r.clear();
    T = 0;
    const size_t colon = s.find(':');
    if (colon != std::string::npos) { T = atoi(s.c_str()); s = s.substr(colon + 1); }
    size_t pos = 0;
    while (pos < s.size()) {
        r.push_back(atoi(s.c_str() + pos));
        const size_t c = s.find(',', pos);
        if (c == std::string::npos) break;
        pos = c + 1;
    }
    return !r.empty();
}
static bool pinned(const char* key, std::vector<int>& r, int& T)
{
    const char* e = experiment(key);
    return e && *e && parse_radices(e, r, T);
}

// The rule a factorization passes before a kernel is instantiated with it -- every pin and every wisdom entry is held to it
// here; the searches below keep to it by construction (choose_n calls it, the others enumerate only what passes): at least
// two radices whose product is n; a workgroup of T threads, a multiple of `granule` of at most tmax, that holds the first and
// the last stage with one butterfly per thread; at most 16 points per thread in every stage AT THAT T (16,3,16 on n/16
// threads needs 18: the translation unit would not compile and the plan would stay on the size-generic kernels for good);
// D > 0: the first radix a multiple of D / DD (the fused kernel, whose first stage skips the zero part of the spectrum).
// T is the thread count the kernel runs on: given (fused kernel), or derived here -- the fewest threads that hold the first
// and the last stage (N-stage rows and columns), or every stage (three-stage kernels: one butterfly per thread throughout,
// so the points bound is the largest radix and always holds).
enum Threads { T_GIVEN, T_HOLDS_ENDS, T_HOLDS_EVERY_STAGE };
static bool valid_factorization(int n, const std::vector<int>& r, int& T, Threads how, int granule, int tmax, int D = 0, int DD = 1)
{
    if (r.size() < 2) return false;
    long prod = 1;
    for (int q : r) { if (!is_radix(q)) return false; prod *= q; }
    if (prod != n) return false;
    const int tmin = std::max(n / r[0], n / r.back());
    if (how == T_HOLDS_ENDS) T = round_up(tmin, granule);
    if (how == T_HOLDS_EVERY_STAGE) T = round_up(n / *std::min_element(r.begin(), r.end()), granule);
    if (T < tmin || T < granule || T > tmax || T % granule) return false;
    if (D > 0 && (r[0] * DD) % D) return false;
    return stage_cost(n, r, T).points <= 16;
}

// three stages, one butterfly per thread and stage (MrFftT): n = r0 * r1 * r2, tk interleaved sequences per workgroup,
// at most tmax threads per sequence.  An odd first radix spreads the stage-0 scatter over the LDS banks without an
// index map; an even one costs bank conflicts in that scatter (2-way for 10 and 12 with one sequence, 4- to 16-way with four).
static bool choose3(int n, int tk, int tmax, int r[3], int* threads, const char* env)
{
    auto all_stages = [&](const std::vector<int>& v) { return std::max(n / v[0], std::max(n / v[1], n / v[2])); };
    std::vector<int> cur;
    int T = 0;
    if (pinned(env, cur, T) && cur.size() == 3 && valid_factorization(n, cur, T, T_HOLDS_EVERY_STAGE, 1, tmax)) {
        std::copy(cur.begin(), cur.end(), r);
        *threads = T;
        return true;
    }
    double best = 0;
    int best_min = 0;
    bool found = false;
    cur.clear();
    each_factorization(n, 3, cur, [&](const std::vector<int>& v) {
        if (v.size() != 3 || all_stages(v) > tmax) return;
        double cost = (double)all_stages(v) * (v[0] + v[1] + v[2]);
        if (v[0] % 2 == 0) cost *= (tk > 1) ? 2.0 : ((v[0] == 10 || v[0] == 12) ? 1.25 : 1.5);
        const int mn = std::min(v[0], std::min(v[1], v[2]));
        if (!found || cost < best || (cost == best && mn > best_min)) { best = cost; best_min = mn; found = true; std::copy(v.begin(), v.end(), r); *threads = all_stages(v); }
    });
    return found;
}

// A factorization on T threads with what the rankings look at: the smallest radix (capped, or 0 where it does not count)
// and the lane slots (with the chooser's penalties).  Between equal numbers of stages: the largest smallest radix, then the
// fewest lane slots.
struct Ranked { std::vector<int> r; int T, mn; double cost; };
static bool fewer_slots(const Ranked& a, const Ranked& b) { return a.mn != b.mn ? a.mn > b.mn : a.cost < b.cost; }
static int r0_rank(int r0) { return r0 == 8 ? 0 : r0 == 12 ? 1 : r0 == 16 ? 2 : 3; }

// the first workgroup size from t up (a multiple of 64) at which no thread holds more than 16 points; 0: none up to 1024
static int first_fit(int n, const std::vector<int>& r, int t, StageCost& sc)
{
    for (int T = t; T <= 1024; T += 64)
        if ((sc = stage_cost(n, r, T)).points <= 16) return T;
    return 0;
}

// any number of stages on T threads (MrFftN / FusedPlanN): first radix a multiple of 4, one butterfly per thread in the
// first and the last stage, at most 16 points per thread in between.  Measured over a dozen sizes (profiles/
// r02_k_jit_factorizations.txt): a first radix of 8 -- every thread of a UW/8-thread workgroup loads and transforms its own
// eight inputs -- beats 16 (half the threads idle in the prefetch and in the first stage) by 10-25 %, even at one stage
// more; after that the fewest stages (every stage is an LDS exchange with two workgroup barriers), the fewest lane
// slots, the largest smallest radix.
static bool fused_better(const Ranked& a, const Ranked& b)
{
    if (r0_rank(a.r[0]) != r0_rank(b.r[0])) return r0_rank(a.r[0]) < r0_rank(b.r[0]);
    if (a.r.size() != b.r.size()) return a.r.size() < b.r.size();
    return fewer_slots(a, b);
}
static bool choose_fused_n(int n, int D, int DD, std::vector<int>& out, int* threads)
{
    std::vector<int> cur;
    int T = 0;
    if (pinned("jit_fused", cur, T) && valid_factorization(n, cur, T, T_GIVEN, 64, 1024, D, DD)) { out = cur; *threads = T; return true; }
    Ranked best = {};
    cur.clear();
    each_factorization(n, 5, cur, [&](const std::vector<int>& v) {
        if (v.size() < 2 || (v[0] * DD) % D) return;
        const int tmin = std::max(n / v[0], n / v.back());
        // whole multiples of 256 threads (the waves spread evenly over the four SIMDs, fewer sharpen passes) beat the
        // minimum in 30 of 43 tuner decisions; small workgroups take one wave more than they need
        StageCost sc;
        const int T = first_fit(n, v, tmin > 128 ? round_up(tmin, 256) : round_up(tmin, 64) + 64, sc);
        if (!T) return;
        if (T > 768) sc.slots *= 1.5;                                          // 64-VGPR territory
        if ((n + 4 * T - 1) / (4 * T) > 4) sc.slots *= 1.3;                    // ring rows no longer fit the registers
        const Ranked cand = {v, T, std::min(sc.min_radix, 4), sc.slots};       // radix-2/3 stages: all exchange, hardly any arithmetic
        if (best.r.empty() || fused_better(cand, best)) best = cand;
    });
    if (best.r.empty()) return false;
    out = best.r; *threads = best.T;
    return true;
}

// The chooser's alternatives for the fused kernel, for the plan-time tuner (fftup_plan_create with FFTUP_FLAG_TUNE_PLAN /
// experiment jit_tune=1): the best factorization (by the ranking above, first radix aside) of every (first radix, number of
// stages, thread count) class, at most `max` of them, the chooser's own pick first.
static bool candidate_before(const Ranked& a, const Ranked& b)
{
    if (a.r.size() != b.r.size()) return a.r.size() < b.r.size();
    if (r0_rank(a.r[0]) != r0_rank(b.r[0])) return r0_rank(a.r[0]) < r0_rank(b.r[0]);
    return fewer_slots(a, b);
}
std::vector<FusedCand> fused_candidates(int n, int D, size_t max, int DD)
{
    std::vector<Ranked> classes;
    std::vector<int> cur;
    each_factorization(n, 4, cur, [&](const std::vector<int>& v) {
        if (v.size() < 2 || (v[0] * DD) % D) return;
        // the fewest threads that will do, and from there the next multiple of 256
        StageCost sc;
        int T = first_fit(n, v, round_up(std::max(n / v[0], n / v.back()), 64), sc);
        for (int tries = 0; T && tries < 2; tries++) {
            const Ranked cand = {v, T, std::min(sc.min_radix, 4), sc.slots};
            auto same = std::find_if(classes.begin(), classes.end(), [&](const Ranked& b) { return b.r[0] == v[0] && b.r.size() == v.size() && b.T == T; });
            if (same == classes.end()) classes.push_back(cand);
            else if (fewer_slots(cand, *same)) *same = cand;
            T = T % 256 ? first_fit(n, v, T / 256 * 256 + 256, sc) : 0;
        }
    });
    std::sort(classes.begin(), classes.end(), candidate_before);
    // variety before depth: at most two candidates per (first radix, number of stages)
    std::vector<FusedCand> out;
    for (const auto& b : classes) {
        if (out.size() >= max) break;
        int same = 0;
        for (const auto& o : out) same += (o.r[0] == b.r[0] && o.r.size() == b.r.size());
        if (same < 2) out.push_back({b.T, b.r});
    }
    return out;
}

// any number of stages for the row and column kernels (MrFftNT, XOR index map: no preference for odd first radices):
// one butterfly per thread in the first and the last stage, at most 16 points per thread, T a multiple of `granule`.
static bool n_better(const Ranked& a, const Ranked& b) { return a.r.size() != b.r.size() ? a.r.size() < b.r.size() : fewer_slots(a, b); }
static bool choose_n(int n, int tmax, int granule, std::vector<int>& out, int* threads, const char* env)
{
    std::vector<int> cur;
    int T = 0;
    if (pinned(env, cur, T) && valid_factorization(n, cur, T, T_HOLDS_ENDS, granule, tmax)) { out = cur; *threads = T; return true; }
    Ranked best = {};
    cur.clear();
    each_factorization(n, 5, cur, [&](const std::vector<int>& v) {
        int T = 0;
        if (!valid_factorization(n, v, T, T_HOLDS_ENDS, granule, tmax)) return;
        const StageCost sc = stage_cost(n, v, T);
        // rows (one sequence per workgroup): no radix-2/3 stage if it can be avoided (3584 = 8*8*8*7 runs 15 % faster than
        // 16*2*7*16); columns: the fewest lane slots decide (four sequences per workgroup: the block size is what hurts)
        const Ranked cand = {v, T, granule >= 64 ? std::min(sc.min_radix, 4) : 0, sc.slots};
        if (best.r.empty() || n_better(cand, best)) best = cand;
    });
    if (best.r.empty()) return false;
    out = best.r; *threads = best.T;
    return true;
}

// What the plan-time tuner found on an MI355X (tools/gpu_wisdom.py, profiles/r02_o_wisdom_mi355x.txt: 107 row lengths x
// factors, frames overlapping on three streams) where it differed from the chooser's pick by more than 3 %: row length,
// D = 2 x upscale factor, "threads:radices".  Consulted after the user's wisdom.txt, for both precisions.
static const struct { int uw, d; const char* plan; } kBuiltinWisdom[] = {
    {768, 3, "128:12,8,8"},
    {1080, 3, "256:12,9,10"},
    {1200, 3, "256:12,10,10"},
    {1280, 4, "256:8,10,16"},
    {1280, 5, "192:10,16,8"},
    {1344, 3, "192:12,16,7"},
    {1440, 3, "192:12,10,12"},
    {1500, 3, "192:15,10,10"},
    {1536, 3, "192:12,16,8"},
    {1536, 6, "192:12,16,8"},
    {1600, 4, "256:16,10,10"},
    {1600, 5, "256:10,10,16"},
    {1728, 3, "256:12,12,12"},
    {1800, 5, "256:10,12,15"},
    {1920, 3, "256:12,10,16"},
    {1920, 4, "256:12,10,16"},
    {1920, 6, "256:12,10,16"},
    {2240, 5, "448:5,7,8,8"},
    {2688, 3, "512:12,4,7,8"},
    {2688, 6, "512:12,4,7,8"},
    {2880, 4, "256:12,15,16"},
    {2880, 8, "256:16,12,15"},
    {3200, 5, "448:10,4,10,8"},
    {3200, 8, "512:8,4,10,10"},
    {3200, 10, "448:10,4,10,8"},
    {3600, 10, "512:10,4,9,10"},
    {3840, 3, "256:15,16,16"},
    {3840, 6, "384:12,4,8,10"},
    {4000, 5, "512:10,4,10,10"},
    {4000, 10, "512:10,4,10,10"},
    {4480, 5, "640:10,8,8,7"},
    {4480, 10, "640:10,8,8,7"},
    {4608, 8, "768:8,8,8,9"},
    {4800, 5, "512:10,4,10,12"},
    {5040, 6, "512:12,5,7,12"},
    {5120, 5, "768:10,8,8,8"},
    {5120, 8, "768:8,8,8,10"},
    {5120, 10, "768:10,8,8,8"},
    {5376, 6, "768:12,7,8,8"},
    {5760, 10, "768:10,8,8,9"},
    {6000, 6, "768:12,5,10,10"},
    {6144, 6, "768:12,8,8,8"},
    {8000, 10, "1024:10,8,10,10"},
};

bool read_file(const std::string& path, std::string& out)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[65536];
    size_t n;
    out.clear();
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}

std::string cache_dir()
{
    std::string d;
    if (const char* e = getenv("FFTUP_CACHE_DIR")) d = e;
    else if (const char* x = getenv("XDG_CACHE_HOME")) d = std::string(x) + "/fftup";
    else if (const char* h = getenv("HOME")) d = std::string(h) + "/.cache/fftup";
    else return "";
    // (mkdir -p of the last two components; failures simply disable the disk cache)
    const size_t slash = d.rfind('/');
    if (slash != std::string::npos && slash > 0) (void)mkdir(d.substr(0, slash).c_str(), 0755);
    (void)mkdir(d.c_str(), 0755);
    return d;
}

// plan-time tuner's memory: <cache dir>/wisdom.txt, one "key = value" per line, last one wins
static std::string wisdom_path() { const std::string d = cache_dir(); return d.empty() ? "" : d + "/wisdom.txt"; }
bool wisdom_lookup(const std::string& key, std::string& value)
{
    std::string text;
    const std::string path = wisdom_path();
    if (path.empty() || !read_file(path, text)) return false;
    bool found = false;
    size_t pos = 0;
    while (pos < text.size()) {
        size_t eol = text.find('\n', pos);
        if (eol == std::string::npos) eol = text.size();
        const std::string line = text.substr(pos, eol - pos);
        const size_t eq = line.find(" = ");
        if (eq != std::string::npos && line.compare(0, eq, key) == 0) { value = line.substr(eq + 3); found = true; }
        pos = eol + 1;
    }
    return found;
}
void wisdom_store(const std::string& key, const std::string& value)
{
    const std::string path = wisdom_path();
    if (path.empty()) return;
    if (FILE* f = fopen(path.c_str(), "a")) { fprintf(f, "%s = %s\n", key.c_str(), value.c_str()); fclose(f); }
}

std::string join(const std::vector<int>& v)
{
    std::string s;
    for (size_t i = 0; i < v.size(); i++) s += (i ? ", " : "") + std::to_string(v[i]);
    return s;
}

// the fused kernel of `c` := FusedPlanN<UW, T, 2, wpe, rr, radices...>
void set_fused_n(Choice& c, int T, const std::vector<int>& radices)
{
    c.fused_kind = 2; c.fr = radices; c.fused_t = T; c.fused_rr = true;
    c.fused_wpe = std::max((T + 255) / 256, std::min(T * 2 / 256, 4));         // >= 128 VGPRs; load() relaxes it when the kernel spills
    const size_t xb = kComplex * (size_t)((c.UW + 15) & ~15);
    const int npass = (c.UW + 4 * T - 1) / (4 * T);
    c.fused_lds = (npass <= 4 ? 1 : 2) * xb + 32 * sizeof(float);
}
std::string fused_key(const Choice& c, const std::string& arch)
{
    return "fused v1 " + arch + " " + std::to_string(c.UW) + " " + std::to_string(c.D) + (c.DD != 1 ? "/" + std::to_string(c.DD) : "") + (c.half ? " h" : " f");
}
std::string fused_value(const Choice& c)
{
    if (c.fused_kind == 0) return "pow2";
    if (c.fused_kind == 1) return "mr16";
    return std::to_string(c.fused_t) + ":" + join(c.fr);
}

// Factorizations for a W x H -> (D/2) W x (D/2) H plan.  D = 2 x the upscale factor: even = integer factor U = D/2
// (polyphase column pass), odd = half-integer factor.  false: some dimension has no supported factorization (the plan
// then stays on the size-generic kernels).  ct_radices: the stage list of the size-generic plan for the output width
// (radices <= 8); arch: device + mode key of the tuner's wisdom file ("" = built-in wisdom only); use_wisdom = false: the
// structural default (pow2 / 16*16*R / the chooser's pick), whatever the wisdom says -- the tuner times it as a candidate.
bool choose(int W, int H, int D, bool half, const std::vector<int>& ct_radices, Choice& c, const std::string& arch, bool use_wisdom, int DD)
{
    // (DD = 2 / 4: quarter- / eighth-integer factor D / 4, D / 8, D odd -- like the half-integer ones one spectrum buffer with all rows, U = 1)
    const int U = (DD == 1 && D % 2 == 0) ? D / 2 : 1;
    c.W = W; c.H = H; c.U = U; c.D = D; c.DD = DD; c.UW = D * W / (2 * DD); c.UH = D * H / (2 * DD); c.half = half;
    if (W < 64 || H < 64 || W > 8192 || H > 8192 || D < 3 || c.UW > 8192 || (D * W) % (2 * DD) || (D * H) % (2 * DD)) return false;
    {   // (the factor D / (2 DD) in lowest terms as far as DD goes, above 1)
        int a = D, b = DD;
        while (b) { const int t = a % b; a = b; b = t; }
        if (DD < 1 || DD > 7 || (DD != 1 && (a != 1 || D <= 2 * DD))) return false;
    }
    if (c.UW % 4) return false;        // the sharpen works on quads of pixels (-u 5 with W = 2 * odd: the size-generic kernels)
    // ---- row R2C
    if (is_pow2(W) && W >= 256) { c.row_kind = 0; c.row_block = W / 8; }
    else if (!experiment("jit_row_nstage") && choose3(W, 1, 1024, c.rr, &c.row_t, "jit_row")) { c.row_kind = 1; c.row_t = round_up(c.row_t, 64); c.row_block = c.row_t; }
    else if (choose_n(W, 1024, 64, c.rn, &c.row_t, "jit_row")) { c.row_kind = 3; c.row_block = c.row_t; }
    else c.row_kind = 2;               // no supported factorization: the size-generic row kernel (same S1 layout) stays
    // ---- column (four columns of a spectrum tile per workgroup; two when a stage of a long column needs more than 256 threads)
    // (columns beyond 5120 points: four of them no longer fit the 160 KB of LDS side by side -- two per workgroup, up to 8192 points)
    auto col_lds = [](int len, int cols) { return kComplex * (size_t)((len * cols + 15) & ~15); };
    auto col_n = [&](int len, std::vector<int>& r, int* tpc, const char* env) {
        if (col_lds(len, 4) <= kLdsMax && choose_n(len, 256, 16, r, tpc, env)) return 4;
        if (col_lds(len, 2) <= kLdsMax && choose_n(len, 512, 32, r, tpc, env)) return 2;
        return 0;
    };
    if (U == 1) {
        int ti = 0;
        if (c.UH > 8192) return false;
        const int cf = col_n(H, c.cn, &c.col_tpc, "jit_col"), ci = col_n(c.UH, c.ci, &ti, "jit_coli");
        if (!cf || !ci) return false;
        c.col_cols = std::min(cf, ci);
        c.col_tpc = std::max(c.col_tpc, ti);
        c.col_kind = 5; c.col_block = c.col_cols * c.col_tpc; c.col_lds = col_lds(c.UH, c.col_cols);
        if (c.col_block > 1024 || c.col_lds > kLdsMax) return false;
    } else if (U > 2) {
        if (!(c.col_cols = col_n(H, c.cn, &c.col_tpc, "jit_col"))) return false;
        c.col_kind = 4; c.col_block = c.col_cols * c.col_tpc; c.col_lds = col_lds(H, c.col_cols);
    } else if (is_pow2(H) && H >= 128 && H <= 2048) {
        c.col_kind = 0; c.col_block = 4 * H / 8; c.col_lds = col_lds(H, 4);      // lswz_size
    } else if (!experiment("jit_col_nstage") && col_lds(H, 4) <= kLdsMax && choose3(H, 4, 256, c.cr, &c.col_tpc, "jit_col")) {
        c.col_kind = 1; c.col_block = 4 * c.col_tpc; c.col_lds = kComplex * (size_t)H * 4;
    } else if ((c.col_cols = col_n(H, c.cn, &c.col_tpc, "jit_col"))) {
        c.col_kind = 3; c.col_block = c.col_cols * c.col_tpc; c.col_lds = col_lds(H, c.col_cols);
    } else return false;
    // ---- fused C2R + sharpen
    const int UW = c.UW;
    size_t xb = kComplex * (size_t)((UW + 15) & ~15);                          // lswz_size(UW)
    int nbuf = 2;
    if ((UW == 1024 || UW == 2048 || UW == 4096) && (8 * DD) % D == 0) { c.fused_kind = 0; c.fused_t = UW / 8; nbuf = 3; }
    else {
        const bool mr16 = UW % 256 == 0 && is_radix(UW / 256) && (16 * DD) % D == 0 && !experiment("jit_fused");
        if (mr16) {
            c.fused_kind = 1; c.fused_t = 256;
            xb = (kComplex * (size_t)(UW + (UW >> 4) + 1) + 15) & ~(size_t)15;                                     // lpad_size(UW)
        } else if (choose_fused_n(UW, D, DD, c.fr, &c.fused_t)) {
            set_fused_n(c, c.fused_t, std::vector<int>(c.fr));
            if (const char* e = experiment("jit_fused_opt")) { int w = 0, r = 1; if (sscanf(e, "%d,%d", &w, &r) == 2) { c.fused_wpe = std::max(1, w); c.fused_rr = r != 0; } }
        } else return false;
    }
    {
        const int npass = (UW + 4 * c.fused_t - 1) / (4 * c.fused_t);
        const size_t nx = (npass <= 4 && (c.fused_kind != 2 || c.fused_rr)) ? 1 : 2;    // FusedGLds::RR
        c.fused_lds = (nx + (nbuf == 3 ? 1 : 0)) * xb + (nbuf == 3 ? 0 : 32 * sizeof(float));
        if (c.fused_lds > kLdsMax) return false;
    }
    // what the plan-time tuner found best on this device for rows of this length (wisdom.txt)
    if (use_wisdom && !experiment("jit_fused")) {
        std::string w;
        bool have = !arch.empty() && wisdom_lookup(fused_key(c, arch), w);
        if (!have && !experiment("jit_no_builtin_wisdom"))
            for (const auto& e : kBuiltinWisdom)
                if (e.uw == UW && e.d == D && DD == 1) { w = e.plan; have = true; }
        if (have && w != fused_value(c) && w != "pow2" && w != "mr16") {
            // (a hand-edited or stale entry must pass the chooser's own rule)
            int T = 0;
            std::vector<int> r;
            if (parse_radices(w.c_str(), r, T) && valid_factorization(UW, r, T, T_GIVEN, 64, 1024, D, DD) && kComplex * (size_t)UW * 2 + 1024 <= kLdsMax) set_fused_n(c, T, r);
        }
    }
    // ---- stand-alone C2R for the pre-sharpen tap (LDS ping-pong, compile-time radices)
    c.ct = ct_radices;
    c.ct_t = std::min(1024, std::max(64, (UW / 8 + 63) / 64 * 64));
    c.ct_lds = 2 * kComplex * (size_t)(UW + (UW >> 4) + 1);
    return true;
}

std::string describe(const Choice& c)
{
    std::string s = (c.DD == 3 || c.DD >= 5) ? "u" + std::to_string(c.D % 2 ? c.D : c.D / 2) + "/" + std::to_string(c.D % 2 ? 2 * c.DD : c.DD) + " row "
                    : c.DD == 4 ? "u" + std::to_string(c.D / 8) + "." + std::to_string(c.D % 8 * 125) + " row "
                    : c.DD == 2 ? "u" + std::to_string(c.D / 4) + (c.D % 4 == 1 ? ".25 row " : ".75 row ")
                    : c.D == 4 ? "row " : (c.D % 2 ? "u" + std::to_string(c.D / 2) + ".5 row " : "u" + std::to_string(c.U) + " row ");
    auto star = [](const std::vector<int>& v) { std::string t; for (size_t i = 0; i < v.size(); i++) t += (i ? "*" : "") + std::to_string(v[i]); return t; };
    s += c.row_kind == 2 ? "generic" : c.row_kind == 0 ? "pow2/8" : c.row_kind == 3 ? star(c.rn) : std::to_string(c.rr[0]) + "*" + std::to_string(c.rr[1]) + "*" + std::to_string(c.rr[2]);
    s += " x" + std::to_string(c.row_block) + ", col ";
    s += c.col_kind == 0 ? ((c.H == 1024 || c.H == 512 || c.H == 256) ? "pow2/8 digit-swap" : "pow2/8") : c.col_kind == 5 ? star(c.cn) + " -> " + star(c.ci) : c.col_kind >= 3 ? star(c.cn) : std::to_string(c.cr[0]) + "*" + std::to_string(c.cr[1]) + "*" + std::to_string(c.cr[2]);
    s += " x" + std::to_string(c.col_block) + (c.col_kind >= 3 && c.col_cols == 2 ? " (2 columns)" : "") + ", fused ";
    if (c.fused_kind == 0) s += "pow2/8";
    else if (c.fused_kind == 1) s += "16*16*" + std::to_string(c.UW / 256);
    else for (size_t i = 0; i < c.fr.size(); i++) s += (i ? "*" : "") + std::to_string(c.fr[i]);
    s += " x" + std::to_string(c.fused_t) + " (" + std::to_string(c.fused_lds) + " B LDS";
    if (c.fused_kind == 2) s += ", " + std::to_string(c.fused_wpe) + " waves/SIMD" + (c.fused_rr ? "" : ", ring rows in LDS");
    s += ")";
    return s;
}

}  // namespace fftup_jit
