// plan_rules.cpp -- the planner without a device (plan_rules.hpp): request checks, then every decision of a plan
#include "plan_rules.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include <hip/hip_fp16.h>

#include "mirror_tables.hpp"
#include "view_tables.hpp"

using namespace fftup;
using Four = PlanGeometry::Four;

static constexpr size_t LDS_GFX950 = (size_t)160 * 1024;      // LDS per workgroup the request checks assume (before any device access)

bool is_smooth(uint32_t n)
{
    if (n == 0) return false;
    for (uint32_t p : {2u, 3u, 5u, 7u})
        while (n % p == 0) n /= p;
    return n == 1;
}

// Four-step split of a row of n points that does not fit the LDS (k_row4_a / k_row4_b): n = n1 * n2.  Pass A transforms tka
// sequences of n1 points side by side -- tka consecutive elements of the row per piece it reads and of the transposed row per
// piece it writes -- pass B tkb sequences of n2 points (tkb consecutive output elements per piece): each the widest of 16, 8, 4, 2, 1
// that divides the other factor and whose two Stockham buffers fit 160 KB.  Widest tiles first (8-byte pieces are a quarter
// of the bandwidth of 32-byte ones, profiles/r05_*_four_step.txt), then as square as possible.
static bool split_four(uint32_t n, size_t el, int* n1, int* n2, int* tka, int* tkb)
{
    long best = -1;
    auto widest = [&](uint32_t len, uint32_t other) -> int {        // sequences of `len` points, tile width must divide `other`
        for (int t : {16, 8, 4, 2, 1})
            if (other % (uint32_t)t == 0 && 2 * el * (size_t)lpad_size((int)len * t) <= LDS_GFX950) return t;
        return 0;
    };
    for (uint32_t d = 2; d * d <= n; d++) {
        if (n % d) continue;
        const uint32_t a = d, b = n / d;                     // a <= b
        const int ta = widest(a, b), tb = widest(b, a);
        if (!ta || !tb) continue;
        // time ~ bytes / piece width: pass A reads and writes the row in pieces of ta elements, pass B writes it in pieces of tb
        const long score = (long)(2000 / ta + 1000 / tb) * (1l << 32) + (long)(b - a);
        if (best < 0 || score < best) { best = score; *n1 = (int)a; *n2 = (int)b; *tka = ta; *tkb = tb; }
    }
    return best >= 0;
}

// radix sequence: as many 8s as possible, then 4/2, then 3,5,7 (VkFFTScheduler vkFFT.h:4707-5189
// makes the same kind of choice; order only affects speed)
StagePlan make_stage_plan(uint32_t n)
{
    StagePlan p{};
    p.n = (int)n;
    uint32_t m = n;
    int e2 = 0;
    while (m % 2 == 0) { m /= 2; e2++; }
    int ns = 0;
    while (e2 >= 3) { p.radix[ns++] = 8; e2 -= 3; }
    if (e2 == 2) p.radix[ns++] = 4;
    if (e2 == 1) p.radix[ns++] = 2;
    for (uint32_t q : {3u, 5u, 7u})
        while (m % q == 0) { p.radix[ns++] = (uint8_t)q; m /= q; }
    p.nstages = ns;
    return p;
}

std::vector<int> stage_radices(const StagePlan& p)
{
    std::vector<int> r;
    for (int s = 0; s < p.nstages; s++) r.push_back(p.radix[s]);
    return r;
}

// ---- FFTUP_FLAG_ANY_SIZE: lengths with a prime factor above 7 run as Bluestein transforms (kernels_bluestein.hpp)
static constexpr uint32_t BZ_MAX_N = 4096;      // the longest such length: L = 8192 >= 2 N - 1 always exists and its buffers fit
// do two LDS buffers of `points` complex fp32 points share the 160 KB of a gfx950 compute unit?
static bool two_buffers_fit(size_t points) { return 2 * sizeof(float2) * (size_t)lpad_size((int)points) <= LDS_GFX950; }
// the smallest 2,3,5,7-smooth length >= 2n - 1 whose two buffers of L * tk points fit (0: none)
static uint32_t bluestein_length(uint32_t n, int tk)
{
    for (uint32_t L = 2 * n - 1; two_buffers_fit((size_t)L * tk); L++)
        if (is_smooth(L)) return L;
    return 0;
}
// length of the LDS sequences the transform of n points works on with tiles of tk: n, its Bluestein length, or 0 (does not fit)
static uint32_t lds_length(uint32_t n, int tk)
{
    if (!is_smooth(n)) return bluestein_length(n, tk);
    return two_buffers_fit((size_t)n * tk) ? n : 0;
}
// column tile width of a plan with a Bluestein column transform: the widest of 8, 4, 2, 1 at which both column transforms fit
// with the SMALLEST L (a wider tile beats a longer L: the row kernels read and write pieces of tk elements); 0: none
static int bluestein_col_tk(uint32_t H, uint32_t uH)
{
    for (int tk : {8, 4, 2, 1})
        if (lds_length(H, tk) && lds_length(uH, tk)) return tk;
    return 0;
}
// the convolution length of a view plan's axis N -> M: mirror plans convolve over the doubled period
static uint32_t view_conv_length(uint32_t N, uint32_t M, bool mirror)
{
    return mirror ? fftup_viewtab::mirror_conv_length(N, M) : fftup_viewtab::conv_length(N, M);
}
// column tile width of a view plan: the widest of 8, 4, 2, 1 at which max(H, its Bluestein length, L_y) * TK fits twice; 0: none
static int view_col_tk(uint32_t H, uint32_t uH, bool mirror)
{
    const uint32_t Ly = view_conv_length(H, uH, mirror);
    for (int tk : {8, 4, 2, 1})
        if (lds_length(H, tk) && two_buffers_fit((size_t)std::max(lds_length(H, tk), Ly) * tk)) return tk;
    return 0;
}

// the sharpen constants reach the reference's shader as "%f" text (VkResample.cpp:893-901, 920)
float const_via_percent_f(double v, bool half)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%f", v);
    float f = (float)strtod(buf, nullptr);
    if (half) f = __half2float(__float2half_rn(f));
    return f;
}

static int round_up(int v, int m) { return (v + m - 1) / m * m; }
// threads of a workgroup whose LDS sequences hold `points` points in all: one per eight points, whole waves, at most `tmax`
static int fft_threads(int points, int tmax) { return std::min(tmax, std::max(64, round_up(points / 8, 64))); }
// The four-step plan of a transform of n points (split_four): the factors' radix lists, LDS bytes and threads of both passes.
// false: no split fits the LDS
static bool make_four(const PlanGeometry& G, Four& f, uint32_t n)
{
    f.on = split_four(n, G.csz, &f.n1, &f.n2, &f.tka, &f.tkb);
    if (!f.on) return false;
    f.p1 = make_stage_plan((uint32_t)f.n1); f.p2 = make_stage_plan((uint32_t)f.n2);
    f.ldsA = 2 * G.csz * (size_t)lpad_size(f.n1 * f.tka); f.ldsB = 2 * G.csz * (size_t)lpad_size(f.n2 * f.tkb);
    const int tmax = kernels_generic_max_threads(G.dbl);
    f.thrA = fft_threads(f.n1 * f.tka, tmax); f.thrB = fft_threads(f.n2 * f.tkb, tmax);
    return true;
}

// Threads a workgroup needs to run every stage of `sp` in place on `tk` interleaved sequences with `pt` points per thread
// (stage_fits_inplace_tk; at least one eighth of the points: the loads and stores around the transform), a multiple of 64 --
// or 0 when that is more than `tmax`.  Radices 3, 5, 7 need more threads than N / 8: one butterfly of 5 or 7 per thread.
static int inplace_threads(const StagePlan& sp, int tk, int pt, int tmax)
{
    long need = (long)sp.n * tk / 8;
    for (int st = 0; st < sp.nstages; st++) {
        const int r = sp.radix[st], per = pt / r;
        if (per < 1) return 0;
        need = std::max(need, ((long)(sp.n / r) * tk + per - 1) / per);
    }
    const long thr = std::max(64l, (need + 63) / 64 * 64);
    return thr <= tmax ? (int)thr : 0;
}

// Rows of n points in LDS (gfx950: 160 KB per workgroup) -- 2: two Stockham buffers, 1: one buffer, in place, 0: not at all.
// Non-R2C rows whose two buffers do not fit run in ONE buffer (fft_lds_inplace: up to 16 384 complex fp32 points, 1024 threads,
// every stage N/R <= (16/R) * 1024: radix 7 up to 14336 points, 3 and 5 up to 15360); the reference switches to multi-upload
// plans there (vkFFT.h:4773-4992)
static int rows_fit(uint32_t n, bool dbl)
{
    const size_t el = dbl ? 16 : 8;
    if (2 * el * (size_t)lpad_size((int)n) <= LDS_GFX950) return 2;
    if (dbl || el * (size_t)lpad_size((int)n) > LDS_GFX950) return 0;
    const StagePlan sp = make_stage_plan(n);
    for (int st = 0; st < sp.nstages; st++)
        if (!stage_fits_inplace((int)n, sp.radix[st], 1024, 16)) return 0;
    return 1;
}

static bool jit_enabled()
{
    const char* e = getenv("FFTUP_JIT");
    return !e || atoi(e) != 0;
}
// The upscale factor as D / (2 DD) when the specialised kernels' assumptions hold: an integer or half-integer factor in [1.5, 8]
// (DD = 1, D = 2u), a quarter-integer one (DD = 2, D = 4u odd: -u 1.25, 1.75, 2.25 ...; round 5), an odd number of eighths (DD = 4: -u 1.125, 1.875)
// or a ratio with denominator 3, 5 or 7 (DD: -u 4/3, 5/3, 1.4, 1.6 ...), output sizes exactly u W and u H,
// and the reference's zero-padding guard of the column pass (float arithmetic, VkResample.cpp:1494-1495) exactly
// [H/2, uH - H/2).  Returns D (0: none of that) and sets *DD.
int jit_factor(float upscale, uint32_t W, uint32_t H, uint32_t uW, uint32_t uH, int zly, int zry, int* DD)
{
    // denominators in the order of their use; lowest terms follow from taking the first that fits (2 DD uW = D W rules out the rest).
    // A factor that is no binary fraction (4/3, 1.6 ...) is whatever float the caller passed: it joins when the reference's float
    // arithmetic makes the output sizes come out exact for THIS size (-u 1.3333334 at 1920x1080 does); the guard may sit a row off
    // the symmetric one (-u 1.2 at 1600x900: [449, 630)): k_col_pad takes it as it is
    *DD = 1;
    for (int dd : {1, 2, 4, 3, 5, 7}) {
        const float t = 2.0f * (float)dd * upscale;
        const int d = (int)lrintf(t);
        if (fabsf(t - (float)d) > 1e-5f * t) continue;
        if (d < 3 || d > 16 * dd || d <= 2 * dd - (dd == 1)) continue;
        if (2 * (uint64_t)dd * uW != (uint64_t)d * W || 2 * (uint64_t)dd * uH != (uint64_t)d * H) continue;
        // integer factors run the polyphase column kernels (k_col_u: residues of the symmetric guard only); every other factor runs
        // k_col_pad, which takes the guard as the reference's float arithmetic puts it -- as long as it leaves the halves apart
        const bool polyphase = dd == 1 && d % 2 == 0;
        if (polyphase ? (zly != (int)(H / 2) || zry != (int)(uH - H / 2)) : (zly < 1 || zly > (int)H || zry < zly || zry > (int)uH)) return 0;
        *DD = dd;
        return d;
    }
    return 0;
}

uint32_t scaled_length(float upscale, uint32_t n) { return (uint32_t)(upscale * (float)n); }
// (float math, uint32 store, exactly as launchResample computes it)
void column_guard(float u, uint32_t uH, int* zly, int* zry)
{
    *zly = (int)(uint32_t)((float)uH / (2 * u));
    *zry = (int)(uint32_t)((2 * u - 1) * (float)uH / (2 * u));
}

int lane_count()
{
    int nl = 3;
    if (const char* e = getenv("FFTUP_STREAMS")) nl = atoi(e);
    return std::max(1, std::min(nl, 4));
}
// Do consecutive frames of this plan overlap on several streams?  A ring of slots (fftup_execute_ring, fftup_submit_rgb8) or
// FFTUP_FLAG_OVERLAP_ITERATIONS (fftup_execute's extension) -- as long as there is more than one stream.
static bool frames_overlap(const PlanGeometry& G)
{
    return lane_count() > 1 && (G.ring > 1 || (G.cfg.flags & FFTUP_FLAG_OVERLAP_ITERATIONS));
}
// (... overlap: what fits beside a strip decides; one after the other: the kernel's own time decides)
std::string wisdom_device_key(const PlanGeometry& G, const DeviceFacts& dev)
{
    return dev.arch + (frames_overlap(G) ? " overlapped" : " sequential");
}

// threads of the fused C2R+sharpen kernel
static int fused_threads(const PlanGeometry& G, const fftup_jit::Choice* jit) { return G.tuned ? (int)G.uW / 8 : (G.mixed == 3 && jit) ? jit->fused_t : 256; }

// Row pairs per workgroup (strip) of the fused C2R+sharpen kernel -- a property of the PLAN (results depend on the cuts in
// their last bits, tests/test_gpu_parity.py: test_fused_output_independent_of_strip_length), chosen by how its frames run.
// Frames that overlap on several streams: ONE strip per compute unit -- the rest of every unit is left to the row and column
// kernels of the frames on the other streams, and the frame time is what counts.
// Frames that run one after the other (a plan without a ring: fftup_execute's ordered iterations, the CLI's -n N):
// nothing runs beside a strip, and a workgroup of at most 512 threads (one or two waves per SIMD) does not hide its own
// latencies: two strips per unit (1080p 100 -> 91 us per iteration, 1000x1000 75 -> 62, 2048x1024 77.2 -> 76.0, -p 2
// 82.7 -> 79.7; 768 and 1024 threads: 2-7 % slower with two; profiles/r04_s_strips_per_unit_sequential.txt).
// How many workgroups are resident is the hardware's business.
int strip_length(const PlanGeometry& G, const DeviceFacts& dev, int fused_threads)
{
    int per_cu = (!frames_overlap(G) && fused_threads <= 512) ? 2 : 1;
    if (const char* e = fftup_jit::experiment("g_per_cu")) per_cu = std::max(1, std::min(4, atoi(e)));
    const int total_pairs = 3 * (int)G.uH / 2, slots = std::max(1, dev.compute_units) * per_cu;
    int pairs = std::max(2, (total_pairs + slots - 1) / slots);
    if (G.u8out) {
        // fused 8-bit store: strips per plane, the three planes' strips of the same rows on ONE of the 8 XCDs (fused_grid):
        // whole triples per XCD, or one compute unit of an XCD gets two strips and the launch takes twice as long
        const int per_xcd = std::max(3, slots / 8) / 3, ppp = (int)G.uH / 2;
        pairs = std::max(2, (ppp + 8 * per_xcd - 1) / (8 * per_xcd));
    }
    if (const char* e = fftup_jit::experiment("pairs_per_strip")) pairs = std::max(1, atoi(e));
    return pairs;
}

// ------------------------------------------------------------------------------------------------ plan_check
// the rules of one view, shared by plan creation and fftup_plan_set_view
int check_view(const char* who, const fftup_view* v, uint32_t uW, uint32_t uH)
{
    if (!std::isfinite(v->origin_x) || !std::isfinite(v->origin_y) || !std::isfinite(v->span_x) || !std::isfinite(v->span_y))
        return fail(FFTUP_E_INVALID_ARG, std::string(who) + ": origin and span must be finite numbers");
    const double sx = v->span_x / (double)uW, sy = v->span_y / (double)uH;
    if (!(sx >= 1.0 / 64 && sx <= 8.0)) return fail(FFTUP_E_INVALID_ARG, std::string(who) + ": the step span_x / out_width must lie in [1/64, 8]");
    if (!(sy >= 1.0 / 64 && sy <= 8.0)) return fail(FFTUP_E_INVALID_ARG, std::string(who) + ": the step span_y / out_height must lie in [1/64, 8]");
    return FFTUP_OK;
}
float view_factor(const fftup_view& v, uint32_t uW, uint32_t uH)
{
    return (float)std::sqrt((double)uW * (double)uH / (v.span_x * v.span_y));
}

static int check_config(const fftup_config& c)
{
    if (c.channels != 3) return fail(FFTUP_E_INVALID_ARG, "channels must be 3 (VkResample.cpp:1368)");
    if (c.precision > 2) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "precision must be 0 (single), 1 (double) or 2 (half)");
    // the float -> uint32 casts of the sizes are undefined for NaN / out-of-range products: bound the inputs first
    // FFTUP_FLAG_DOWNSCALE: factors in [1/8, 1) instead (a factor below 1 without the flag stays an error)
    const bool down = (c.flags & FFTUP_FLAG_DOWNSCALE) != 0;
    if (down && !(c.upscale >= 0.125f && c.upscale < 1.0f)) return fail(FFTUP_E_INVALID_ARG, "FFTUP_FLAG_DOWNSCALE: the factor must lie in [0.125, 1)");
    if (!down && !(c.upscale >= 1.0f && c.upscale <= 64.0f)) return fail(FFTUP_E_INVALID_ARG, "upscale must be a finite number in [1, 64]");
    if (c.width > (1u << 16) || c.height > (1u << 16)) return fail(FFTUP_E_INVALID_ARG, "width/height above 65536");
    if (c.ring > 1024) return fail(FFTUP_E_INVALID_ARG, "ring must be <= 1024");
    if (!(c.sharpen == c.sharpen)) return fail(FFTUP_E_INVALID_ARG, "sharpen is NaN");
    return FFTUP_OK;
}

// fftup_plan_create_view: every rule of such a plan (the bounds of the other plan kinds do not apply)
static int check_view_request(const fftup_config& c, const fftup_view* view, uint32_t uW, uint32_t uH)
{
    const uint32_t W = c.width, H = c.height;
    if (W < 2 || H < 2 || uW < 2 || uH < 2) return fail(FFTUP_E_INVALID_ARG, "fftup_plan_create_view: every length (width, height, out_width, out_height) must be at least 2");
    if (int rc = check_view("fftup_plan_create_view", view, uW, uH)) return rc;
    if (c.precision == 1) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "fftup_plan_create_view plans exist for -p 0 and -p 2");
    if (c.flags & FFTUP_FLAG_DCT) return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view covers the FFT mode only (no FFTUP_FLAG_DCT)");
    if (W > 8192u) return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view: rows of at most 8192 points (no non-R2C or four-step path)");
    const bool mirror = (c.flags & FFTUP_FLAG_MIRROR) != 0;
    if (mirror && (2 * (uint64_t)W + uW > 8192u || fftup_viewtab::mirror_conv_length(W, uW) > 8192u))
        return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_MIRROR: the row convolution length (2,3,5,7-smooth, at least 2 width + out_width) must be at most 8192");
    if (!mirror && (2 * (uint64_t)(W / 2) + uW > 8192u || fftup_viewtab::conv_length(W, uW) > 8192u))
        return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view: the row convolution length (2,3,5,7-smooth, at least 2 (width/2) + out_width) must be at most 8192");
    for (uint32_t n : {W, H}) {
        if (!is_smooth(n) && !(c.flags & FFTUP_FLAG_ANY_SIZE))
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view: width and height must factor into 2,3,5,7; FFTUP_FLAG_ANY_SIZE accepts any length up to 4096");
        if (!is_smooth(n) && n > BZ_MAX_N)
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_ANY_SIZE: " + std::to_string(n) + " has a prime factor above 7 and is longer than 4096");
    }
    if (mirror && (2 * (uint64_t)H + uH > 16384u || !view_col_tk(H, uH, true)))
        return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_MIRROR: the columns must fit the LDS (two buffers of the column convolution length, at least 2 height + out_height, at a tile width of 1)");
    if (!mirror && (2 * (uint64_t)(H / 2) + uH > 16384u || !view_col_tk(H, uH, false)))
        return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view: the columns must fit the LDS (two buffers of the column convolution length at a tile width of 1)");
    return FFTUP_OK;
}

// fftup_plan_create_size: each axis on its own, up, down or equal, either parity
static int check_size_request(const fftup_config& c, uint32_t uW, uint32_t uH, uint32_t align)
{
    const uint32_t W = c.width, H = c.height;
    if (W < 2 || H < 2 || uW < 2 || uH < 2) return fail(FFTUP_E_INVALID_ARG, "fftup_plan_create_size: every length (width, height, out_width, out_height) must be at least 2");
    if (align > FFTUP_ALIGN_CENTRE) return fail(FFTUP_E_INVALID_ARG, "fftup_plan_create_size: align must be FFTUP_ALIGN_CORNER (0) or FFTUP_ALIGN_CENTRE (1)");
    if (8 * (uint64_t)uW < W || uW > 8 * (uint64_t)W) return fail(FFTUP_E_INVALID_ARG, "fftup_plan_create_size: out_width must lie in [width/8, 8 width]");
    if (8 * (uint64_t)uH < H || uH > 8 * (uint64_t)H) return fail(FFTUP_E_INVALID_ARG, "fftup_plan_create_size: out_height must lie in [height/8, 8 height]");
    return FFTUP_OK;
}

// The bounds of the plans that run the Bluestein / odd-size kernels (two-buffer R2C rows, columns in LDS, fp32 arithmetic, no
// DCT), under the wording of the rule that sent the plan there: `who` opens the messages about rows and columns.  max_non_smooth:
// the longest length with a prime factor above 7 (0: such lengths were dealt with already)
static int check_resampled(const PlanGeometry& G, const char* dct_msg, const char* precision_msg, const std::string& who, const char* rows, const char* columns,
                           uint32_t max_non_smooth)
{
    if (G.cfg.flags & FFTUP_FLAG_DCT) return fail(FFTUP_E_UNSUPPORTED_SIZE, dct_msg);
    if (G.cfg.precision == 1) return fail(FFTUP_E_UNSUPPORTED_PRECISION, precision_msg);
    for (uint32_t n : {G.W, G.H, G.uW, G.uH})
        if (max_non_smooth && !is_smooth(n) && n > max_non_smooth)
            return fail(FFTUP_E_UNSUPPORTED_SIZE, who + ": " + std::to_string(n) + " has a prime factor above 7 and is longer than " + std::to_string(max_non_smooth));
    if (G.W > 8192u || G.uW > 8192u) return fail(FFTUP_E_UNSUPPORTED_SIZE, who + ": " + rows + " (no non-R2C or four-step path)");
    if (!bluestein_col_tk(G.H, G.uH)) return fail(FFTUP_E_UNSUPPORTED_SIZE, who + ": " + columns + " (no four-step columns)");
    return FFTUP_OK;
}

// what the modes of a plan exclude, and whether rows of these lengths can run at all (G: sizes and modes set)
static int check_modes(const PlanGeometry& G, bool odd_len)
{
    const uint32_t W = G.W, H = G.H, uW = G.uW, uH = G.uH, flags = G.cfg.flags;
    if (!G.exact && (W < 2 || H < 2 || uW < 2 || uH < 2 || (odd_len && !G.odd) || (!G.down && (uW < W || uH < H))))
        return fail(FFTUP_E_INVALID_ARG, "width/height (and upscaled sizes) must be even, upscale >= 1; FFTUP_FLAG_ODD_SIZE accepts odd lengths");
    if (G.down && (uW < 2 || uH < 2 || uW >= W || uH >= H))
        return fail(FFTUP_E_INVALID_ARG, "FFTUP_FLAG_DOWNSCALE: the output sizes must be at least 2 and below the input's");
    if (G.bz && !(flags & FFTUP_FLAG_ANY_SIZE))
        return fail(FFTUP_E_UNSUPPORTED_SIZE, "sizes must factor into 2,3,5,7 (vkFFT.h:4719-4726); FFTUP_FLAG_ANY_SIZE accepts any even length up to 4096");
    int rc = FFTUP_OK;
    // (the smooth lengths of a Bluestein plan keep their Stockham transforms in the same kernels)
    if (G.bz && !G.view)
        rc = check_resampled(G, "FFTUP_FLAG_DCT plans need sizes that factor into 2,3,5,7 (FFTUP_FLAG_ANY_SIZE covers the FFT modes only)",
                             "FFTUP_FLAG_ANY_SIZE plans with a non-smooth length exist for -p 0 and -p 2", "FFTUP_FLAG_ANY_SIZE",
                             "a plan with a non-smooth length needs rows of at most 8192 points", "a plan with a non-smooth length needs columns that fit the LDS", BZ_MAX_N);
    if (!rc && G.odd && !G.exact)
        rc = check_resampled(G, "FFTUP_FLAG_DCT plans need even sizes (FFTUP_FLAG_ODD_SIZE covers the FFT modes only)",
                             "FFTUP_FLAG_ODD_SIZE plans with an odd length exist for -p 0 and -p 2", "FFTUP_FLAG_ODD_SIZE",
                             "a plan with an odd length needs rows of at most 8192 points", "a plan with an odd length needs columns that fit the LDS", 0);
    if (!rc && G.exact && !G.view)
        rc = check_resampled(G, "fftup_plan_create_size covers the FFT mode only (no FFTUP_FLAG_DCT)", "fftup_plan_create_size plans exist for -p 0 and -p 2",
                             "fftup_plan_create_size", "rows of at most 8192 points", "the columns must fit the LDS", 0);
    if (rc) return rc;
    // DCT plans: fp32 / fp16 storage, rows in one LDS launch (no non-R2C-like path for uW beyond 8192)
    if (G.dct && G.dbl) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "FFTUP_FLAG_DCT plans exist for -p 0 and -p 2");
    if (G.dct && uW > 8192u) return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_DCT plans need an upscaled width of at most 8192");
    // downscale plans: the same storage, the input rows in one two-buffer LDS launch (no four-step or non-R2C downscale)
    if (G.down && G.dbl) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "FFTUP_FLAG_DOWNSCALE plans exist for -p 0 and -p 2");
    if (G.down && W > 8192u) return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_DOWNSCALE plans need an input width of at most 8192");
    // non-R2C rows beyond one buffer run in four steps through HBM (k_row4_a / k_row4_b), as the reference's multi-upload plans
    int a, b, t, t2;
    if (G.cplx && ((!rows_fit(uW, G.dbl) && !split_four(uW, G.csz, &a, &b, &t, &t2)) || (!rows_fit(W, G.dbl) && !split_four(W, G.csz, &a, &b, &t, &t2))))
        return fail(FFTUP_E_UNSUPPORTED_SIZE, "row too long: no four-step split of the row length fits the LDS");
    return FFTUP_OK;
}

int plan_check(const PlanRequest& rq, PlanGeometry& G)
{
    if (!rq.cfg) return fail(FFTUP_E_INVALID_ARG, "null argument");
    G = PlanGeometry{};
    G.cfg = *rq.cfg;
    G.exact = rq.size != nullptr;
    G.view = rq.view != nullptr;
    if (G.exact) {
        // the effective factor u_e = sqrt(uW uH / (W H)) takes the place of cfg->upscale in the sharpen constant (and only there);
        // 1 until the sizes below are known to be valid
        G.cfg.upscale = 1.0f;
        G.cfg.flags &= ~(uint32_t)FFTUP_FLAG_DOWNSCALE;         // (implied per axis: accepted, changes nothing)
    }
    if (int rc = check_config(G.cfg)) return rc;
    if ((G.cfg.flags & FFTUP_FLAG_MIRROR) && !G.view)
        return fail(FFTUP_E_INVALID_ARG, "FFTUP_FLAG_MIRROR is valid on fftup_plan_create_view only (fftup_plan_create and fftup_plan_create_size plans are periodic; FFTUP_FLAG_DCT is their mode without the wrap)");
    const uint32_t W = G.W = G.cfg.width, H = G.H = G.cfg.height;
    const uint32_t uW = G.uW = G.exact ? rq.size[0] : scaled_length(G.cfg.upscale, W);
    const uint32_t uH = G.uH = G.exact ? rq.size[1] : scaled_length(G.cfg.upscale, H);
    if (G.view) {
        if (int rc = check_view_request(G.cfg, rq.view, uW, uH)) return rc;
        G.cfg.upscale = view_factor(*rq.view, uW, uH);
    }
    else if (G.exact) {
        if (int rc = check_size_request(G.cfg, uW, uH, rq.align)) return rc;
        G.cfg.upscale = (float)std::sqrt((double)uW * (double)uH / ((double)W * (double)H));
    }
    G.ring = G.cfg.ring ? G.cfg.ring : 1;
    G.half = G.cfg.precision == 2;
    G.dbl = G.cfg.precision == 1;
    G.esz = G.dbl ? 8 : (G.half ? 2 : 4);
    G.csz = G.dbl ? 16 : 8;
    G.align = G.exact ? rq.align : 0;
    G.down = (G.cfg.flags & FFTUP_FLAG_DOWNSCALE) != 0;
    G.dct = (G.cfg.flags & FFTUP_FLAG_DCT) != 0;
    G.mirror = G.view && (G.cfg.flags & FFTUP_FLAG_MIRROR);
    // FFTUP_FLAG_ODD_SIZE: odd lengths are valid; `odd`: this plan has one (exact trigonometric resampling, kernels_odd.hpp).  A
    // plan whose four lengths are even is the same plan with or without the flag.
    // (fftup_plan_create_size: always that rule, whatever the parities, FFTUP_FLAG_ODD_SIZE implied)
    const bool odd_len = (W & 1) || (H & 1) || (uW & 1) || (uH & 1);
    G.odd = G.exact || (odd_len && (G.cfg.flags & FFTUP_FLAG_ODD_SIZE));
    // FFTUP_FLAG_ANY_SIZE: lengths with a prime factor above 7 run as Bluestein transforms; `bz`: this plan has one.  A plan
    // whose four lengths are smooth is the same plan with or without the flag.
    // (view plans: only the forward transforms have the input's lengths; the output lengths are the chirp-z transforms' business)
    G.bz = !is_smooth(W) || !is_smooth(H) || (!G.view && (!is_smooth(uW) || !is_smooth(uH)));
    // R2C rule of the reference: uW <= maxComputeSharedMemorySize/8 with 64 KB (VkResample.cpp:1424; complexSizeCalc = 16
    // for -p 1, VkResample.cpp:1334-1336, halves the limit); beyond it the full complex path runs
    G.cplx = uW > (G.dbl ? 4096u : 8192u);
    if (int rc = check_modes(G, odd_len)) return rc;
    // (FFT downscale plans keep only the bins the output holds, kx <= uW/2: S1, S2 and the column pass shrink with the output)
    // (odd plans: the bins both lengths hold, kx <= min(W, uW)/2 -- floor: an odd length has (n + 1)/2 bins from 0 up, no Nyquist bin)
    G.ncols = G.cplx ? (int)W : (G.down && !G.dct) ? (int)(uW / 2 + 1) : (int)(W / 2 + 1);
    if (G.odd) G.ncols = (int)(std::min(W, uW) / 2 + 1);
    if (G.view) G.ncols = (int)(W / 2 + 1);             // (the worst case: the buffers hold any view; view_apply sets the current one)
    return FFTUP_OK;
}

// ------------------------------------------------------------------------------------------------ plan_geometry
// column tile width and column LDS of a plan without ahead-of-time kernels: the first of these that applies
static int choose_column_tile(PlanGeometry& G, size_t lds_max)
{
    const uint32_t W = G.W, H = G.H, uW = G.uW, uH = G.uH;
    // u = 2 with the symmetric guard: the polyphase column kernel (k_col_poly: forward, phase, length-H inverse in ONE buffer of
    // H TK points, odd rows out; the C2R kernel takes the even rows from S1) where its stages run in place
    const char* const poly_e = fftup_jit::experiment("generic_poly");
    if (!G.cplx && !G.dct && !G.down && !G.odd && is_smooth(H) && uW == 2 * W && uH == 2 * H && G.zly == (int)(H / 2) && G.zry == (int)(uH - H / 2) && !(poly_e && atoi(poly_e) == 0)) {
        for (int tk : {8, 4, 2, 1}) {
            const size_t need = G.csz * (size_t)lpad_size((int)H * tk);
            const int thr = inplace_threads(G.planH, tk, COL_INPLACE_PT, kernels_generic_max_threads(G.dbl));
            if (thr && need <= lds_max / 2) { G.TK = tk; G.ldsCol = need; G.poly = true; G.thrCol = thr; break; }    // (two workgroups per compute unit)
        }
    }
    // -p 1 R2C plans: ONE buffer where every stage of both column transforms runs in place with COL_INPLACE_PT points per thread (k_col<.., true>)
    if (!G.TK && G.dbl && !G.cplx) {
        for (int tk : {8, 4, 2, 1}) {
            const size_t need = G.csz * (size_t)lpad_size((int)uH * tk);
            const int tmax = kernels_generic_max_threads(true);
            const int thr = std::max(inplace_threads(G.planH, tk, COL_INPLACE_PT, tmax), inplace_threads(G.planUH, tk, COL_INPLACE_PT, tmax));
            const bool ok = inplace_threads(G.planH, tk, COL_INPLACE_PT, tmax) && inplace_threads(G.planUH, tk, COL_INPLACE_PT, tmax) &&
                            need <= lds_max / 2 && (size_t)(H / 2) * tk <= (size_t)COL_INPLACE_PT * thr;  // (two workgroups per compute unit)
            if (ok) { G.TK = tk; G.ldsCol = need; G.inplaceC = true; G.thrCol = thr; break; }
        }
    }
    // a Bluestein column transform: buffers of L * TK points (bluestein_col_tk: checked before any device access); the
    // column kernel of an odd plan is sized the same way, max(length, L) * TK with L = length for a smooth one
    if (G.view) {
        G.viewL[0] = view_conv_length(W, uW, G.mirror); G.viewL[1] = view_conv_length(H, uH, G.mirror);
        G.TK = view_col_tk(H, uH, G.mirror);
        G.ldsCol = 2 * G.csz * (size_t)lpad_size((int)(std::max(lds_length(H, G.TK), G.viewL[1]) * (uint32_t)G.TK));
        if (G.ldsCol > lds_max) return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view: this device's LDS does not hold the column transform");
    }
    if (!G.TK && (G.odd || !is_smooth(H) || !is_smooth(uH))) {
        G.TK = bluestein_col_tk(H, uH);
        G.ldsCol = 2 * G.csz * (size_t)lpad_size((int)(std::max(std::max(H, uH), std::max(lds_length(H, G.TK), lds_length(uH, G.TK))) * (uint32_t)G.TK));
        if (G.ldsCol > lds_max) return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_ANY_SIZE: this device's LDS does not hold the column transform");
    }
    // column tile width: widest of 8,4,2,1 whose ping-pong buffers fit in LDS (downscale plans: the forward transform,
    // length H, is the longer one)
    if (!G.TK) for (int tk : {8, 4, 2, 1}) {
        size_t need = 2 * G.csz * (size_t)lpad_size((int)std::max(H, uH) * tk);
        if (need <= lds_max) { G.TK = tk; G.ldsCol = need; break; }
    }
    return FFTUP_OK;
}

static bool aot_enabled()      // (experiment aot=0: the sizes with ahead-of-time kernels go through the plan-time compiler as well)
{
    const char* const aot_e = fftup_jit::experiment("aot");
    return !(aot_e && atoi(aot_e) == 0);
}

int plan_geometry_columns(PlanGeometry& G, const DeviceFacts& dev)
{
    const uint32_t W = G.W, H = G.H, uW = G.uW, uH = G.uH;
    // zero-padding ranges exactly as launchResample computes them (float math, uint32 store)
    const float u = G.cfg.upscale;
    G.zlx = (int)(W / 2);
    G.zrx = G.cplx ? (int)(uint32_t)((2 * u - 1) * (float)uW / (2 * u)) : (int)(uW / 2);      // VR:1498 / VR:1493
    // (downscale plans have no padding: no guard, and 2u - 1 < 0 would make the cast undefined)
    G.zly = G.zry = 0;
    if (!G.down && !G.exact) column_guard(u, uH, &G.zly, &G.zry);

    G.planW = make_stage_plan(W);
    G.planH = make_stage_plan(H);
    G.planUW = make_stage_plan(uW);
    G.planUH = make_stage_plan(uH);

    // size-specialised kernels: u == 2 and power-of-two sizes with instantiated plans
    const bool aot_u2 = aot_enabled() && !G.dbl && !G.cplx && !G.dct && !G.down && !G.exact && !(G.cfg.flags & FFTUP_FLAG_GENERIC_KERNELS) && uW == 2 * W && uH == 2 * H;
    G.tuned = aot_u2 && (W == 512 || W == 1024 || W == 2048) && (H == 256 || H == 512 || H == 1024);
    G.TK = 0;
    if (G.tuned) {
        G.TK = TUNED_TK;
        G.ldsCol = kernels_tuned_col_lds(H);
    }
    else if (int rc = choose_column_tile(G, dev.lds_bytes)) return rc;
    if (!G.TK && G.dct) return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_DCT: the columns do not fit the LDS (no four-step DCT)");
    if (!G.TK && G.down) return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_DOWNSCALE: the columns do not fit the LDS (no four-step downscale)");
    if (!G.TK) {
        // not even one column fits: tiles of one column, both column transforms in four steps through HBM (k_row4_a / k_row4_b)
        G.TK = 1; G.ldsCol = 0;
        if (!make_four(G, G.colF, H) || !make_four(G, G.colI, uH))
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "column too long: no four-step split of the height fits the LDS");
    }
    if (aot_u2 && !G.tuned && G.TK >= 4) G.mixed = kernels_aot_mixed_plan(W, H);                 // 1920x1080, 1280x720
    if (G.mixed) { G.TK = 4; G.ldsCol = sizeof(float2) * (size_t)H * 4; }                        // k_col_m: one in-place buffer
    return FFTUP_OK;
}

// any other size with an integer or half-integer upscale factor: kernels specialised for it at plan time (the counterpart
// of VkFFT generating its shaders at plan time)
int plan_jit_factor(const PlanGeometry& G, int* DD)
{
    *DD = 1;
    if (G.dbl || G.cplx || G.dct || G.down || G.bz || G.odd || G.tuned || G.mixed || (G.cfg.flags & (FFTUP_FLAG_GENERIC_KERNELS | FFTUP_FLAG_UNFUSED_SHARPEN)) || !jit_enabled())
        return 0;
    return jit_factor(G.cfg.upscale, G.W, G.H, G.uW, G.uH, G.zly, G.zry, DD);
}

// The family, decided here once.  The rules above make the families exclusive wherever two of them could claim a plan (the
// long rows of cplx and the double arithmetic of f64 exist in the size-generic upscale kernels only; the ahead-of-time and
// plan-time kernels take none of the other modes): stated here, so that no order of tests has to be relied on.  Three
// pairs are no conflict: view plans are `odd` and `exact` (they run the odd plans' row kernel), odd plans may be `down`
// (the direction is a parameter of their kernels), DCT plans may be `down` too.
static int choose_family(PlanGeometry& G)
{
    const bool resampled = G.odd || G.view || G.bz, own = G.tuned || G.mixed;
    if ((G.cplx && (G.dct || G.down || resampled)) || (G.dbl && (G.dct || G.down || resampled)) || (G.dct && resampled) ||
        (own && (G.cplx || G.dbl || G.dct || G.down || resampled)) || (G.tuned && G.mixed))
        return fail(FFTUP_E_INVALID_ARG, "internal: the plan rules let two kernel families claim this plan");
    using Family = PlanGeometry::Family;
    G.family = G.cplx ? Family::cplx : G.dbl ? Family::f64 : G.dct ? Family::dct : G.view ? Family::view : G.odd ? Family::odd : G.down ? Family::down
               : G.tuned ? Family::tuned : G.mixed == 3 ? Family::mixed_jit : G.mixed ? Family::mixed_aot : Family::generic;
    return FFTUP_OK;
}

// LDS bytes of the row kernels, in-place and four-step rows
static int row_buffers(PlanGeometry& G, size_t lds_max)
{
    const uint32_t W = G.W, uW = G.uW;
    G.ldsRowF = 2 * G.csz * (size_t)lpad_size((int)W);
    G.ldsRowI = 2 * G.csz * (size_t)lpad_size((int)uW);
    if (G.bz) {                                            // Bluestein rows: buffers of L points
        G.ldsRowF = 2 * G.csz * (size_t)lpad_size((int)lds_length(W, 1));
        G.ldsRowI = 2 * G.csz * (size_t)lpad_size((int)lds_length(uW, 1));
        if (G.ldsRowF > lds_max) return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_ANY_SIZE: this device's LDS does not hold the row transform");
    }
    if (G.cplx) {                                          // long non-R2C rows: one buffer, in place (rows_fit)
        G.inplaceF = rows_fit(W, G.dbl) == 1; G.inplaceI = rows_fit(uW, G.dbl) == 1;
        if (G.inplaceF) G.ldsRowF /= 2;
        if (G.inplaceI) G.ldsRowI /= 2;
        // ... or four steps through HBM (a split exists: plan_check)
        if (!rows_fit(W, G.dbl)) { make_four(G, G.fourF, W); G.ldsRowF = 0; }
        if (!rows_fit(uW, G.dbl)) { make_four(G, G.fourI, uW); G.ldsRowI = 0; }
    }
    if (G.view) G.ldsRowI = 2 * G.csz * (size_t)lpad_size((int)G.viewL[0]);      // (L_x >= out_width)
    if (G.ldsRowI > lds_max) return fail(FFTUP_E_UNSUPPORTED_SIZE, "upscaled width too large for LDS");
    return FFTUP_OK;
}

static void choose_threads(PlanGeometry& G)
{
    const uint32_t W = G.W, H = G.H, uW = G.uW, uH = G.uH;
    const int tmax = kernels_generic_max_threads(G.dbl);
    G.thrW = fft_threads((int)W, tmax);
    G.thrUW = fft_threads((int)uW, tmax);
    if (!(G.poly || G.inplaceC)) G.thrCol = fft_threads((int)std::max(H, uH) * G.TK, tmax);     // (in-place column plans chose theirs with the tile)
    if (G.bz) {                                        // the sequences in LDS are the Bluestein transforms'
        G.thrW = fft_threads((int)lds_length(W, 1), tmax);
        G.thrUW = fft_threads((int)lds_length(uW, 1), tmax);
        if (!G.poly) G.thrCol = fft_threads((int)std::max(lds_length(H, G.TK), lds_length(uH, G.TK)) * G.TK, tmax);
    }
    if (G.view) {                                      // the chirp-z transforms: the sequences hold L points
        G.thrUW = fft_threads((int)G.viewL[0], tmax);
        G.thrCol = fft_threads((int)std::max(lds_length(H, G.TK), G.viewL[1]) * G.TK, tmax);
    }
    // -p 1 R2C rows: one LDS buffer where every stage runs in place with 8 points per thread (two workgroups per compute unit)
    if (G.dbl && !G.cplx) {
        const int tf = inplace_threads(G.planW, 1, 8, tmax), ti = inplace_threads(G.planUW, 1, 8, tmax);
        if (tf) { G.inplaceF = true; G.thrW = tf; G.ldsRowF /= 2; }
        if (ti) { G.inplaceI = true; G.thrUW = ti; G.ldsRowI /= 2; }
    }
}

int plan_geometry_finish(PlanGeometry& G, const DeviceFacts& dev, const fftup_jit::Choice* jit)
{
    if (jit) {
        G.mixed = 3; G.U = jit->U; G.TK = 4; G.ldsCol = jit->col_lds;
        // (inputs taller than 4800 rows: the size-generic plan would have run its columns in four steps through HBM -- the
        // specialised column kernel holds two whole columns in LDS instead)
        G.colF = Four{}; G.colI = Four{};
    }
    if (G.tuned || G.mixed) G.poly = false;               // (their own column kernels)
    if (int rc = choose_family(G)) return rc;
    G.fused = (G.tuned || G.mixed) && !(G.cfg.flags & FFTUP_FLAG_UNFUSED_SHARPEN);
    G.u8out = G.fused && (G.cfg.flags & FFTUP_FLAG_FUSE_U8_STORE);
    G.pairs_per_strip = strip_length(G, dev, fused_threads(G, jit));
    G.NT = (G.ncols + G.TK - 1) / G.TK;
    if (int rc = row_buffers(G, dev.lds_bytes)) return rc;
    choose_threads(G);
    // the Bluestein lengths of W, H, uW, uH (view plans: the output lengths are the chirp-z transforms' business)
    const uint32_t len[4] = {G.W, G.H, G.uW, G.uH};
    for (int i = 0; i < 4; i++)
        if (G.bz && !is_smooth(len[i]) && !(G.view && i >= 2)) G.bzL[i] = lds_length(len[i], (i & 1) ? G.TK : 1);
    G.upsq = const_via_percent_f((double)(G.cfg.upscale * G.cfg.upscale), G.half);   // VkResample.cpp:1615
    G.coef = const_via_percent_f((double)G.cfg.sharpen, G.half);                     // VkResample.cpp:1616
    return FFTUP_OK;
}

// ------------------------------------------------------------------------------------------------ align_geometry
// fftup_align_create: the rules and decisions of an aligner (include/fftup.h), arithmetic on the configuration alone
static uint32_t pow2_floor(uint32_t v)
{
    uint32_t p = 1;
    while (p <= v / 2) p *= 2;
    return v ? p : 0;
}

int align_geometry(const fftup_align_config& c, AlignGeometry& G)
{
    const char* who = "fftup_align_create: ";
    if (c.width == 0 || c.height == 0) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "width and height must be > 0");
    if (c.width > (1u << 16) || c.height > (1u << 16)) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "width/height above 65536");
    if (c.precision == 1) return fail(FFTUP_E_UNSUPPORTED_PRECISION, std::string(who) + "precision must be 0 (float planes) or 2 (half planes): there are no -p 1 frames");
    if (c.precision > 2) return fail(FFTUP_E_UNSUPPORTED_PRECISION, std::string(who) + "precision must be 0 (float planes) or 2 (half planes)");
    if (c.decimate != 0 && c.decimate != 1 && c.decimate != 2 && c.decimate != 4 && c.decimate != 8)
        return fail(FFTUP_E_INVALID_ARG, std::string(who) + "decimate " + std::to_string(c.decimate) + " must be 1, 2, 4 or 8 (0: automatic)");
    const uint32_t win[2] = {c.window_w, c.window_h};
    for (int a = 0; a < 2; a++)
        if (win[a] && (win[a] < 16 || win[a] > 1024 || (win[a] & (win[a] - 1))))
            return fail(FFTUP_E_INVALID_ARG, std::string(who) + (a ? "window_h " : "window_w ") + std::to_string(win[a]) + " must be a power of two in [16, 1024] (0: automatic)");
    if (!(c.band == 0.0f || (c.band > 0.0f && c.band <= 1.0f))) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "band must lie in (0, 1] (0: 0.5)");
    if (c.upsample && (c.upsample < 4 || c.upsample > 64)) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "upsample " + std::to_string(c.upsample) + " must lie in [4, 64] (0: 32)");
    if (c.max_batch > 65535) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "max_batch must be <= 65535");
    G.W = c.width; G.H = c.height; G.precision = c.precision;
    G.band = c.band == 0.0f ? 0.5f : c.band;
    G.kappa = c.upsample ? c.upsample : 32;
    G.max_batch = c.max_batch ? c.max_batch : 16;
    // automatic d: the smallest whose automatic windows are both at most 1024; none: 8, the windows capped
    G.d = c.decimate;
    if (!G.d) {
        G.d = 8;
        for (uint32_t d : {1u, 2u, 4u, 8u})
            if (pow2_floor(c.width / d) <= 1024 && pow2_floor(c.height / d) <= 1024) { G.d = d; break; }
    }
    if (c.width / G.d < 16 || c.height / G.d < 16)
        return fail(FFTUP_E_INVALID_ARG, std::string(who) + "a frame of " + std::to_string(c.width) + "x" + std::to_string(c.height) + " has fewer than 16 decimated pixels on an axis (d = " + std::to_string(G.d) + ")");
    G.nx = c.window_w ? c.window_w : std::min(1024u, pow2_floor(c.width / G.d));
    G.ny = c.window_h ? c.window_h : std::min(1024u, pow2_floor(c.height / G.d));
    if ((uint64_t)G.nx * G.d > c.width) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "window_w * d = " + std::to_string((uint64_t)G.nx * G.d) + " exceeds the frame's width " + std::to_string(c.width));
    if ((uint64_t)G.ny * G.d > c.height) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "window_h * d = " + std::to_string((uint64_t)G.ny * G.d) + " exceeds the frame's height " + std::to_string(c.height));
    G.crop_x = (c.width - G.nx * G.d) / 2;
    G.crop_y = (c.height - G.ny * G.d) / 2;
    G.band_kx = (uint32_t)std::floor((double)G.band * (double)G.nx / 2.0);
    G.band_ky = (uint32_t)std::floor((double)G.band * (double)G.ny / 2.0);
    G.Kx = G.band_kx < G.nx / 2 ? 2 * G.band_kx + 1 : G.nx;
    G.Ky = G.band_ky < G.ny / 2 ? 2 * G.band_ky + 1 : G.ny;
    return FFTUP_OK;
}

// ------------------------------------------------------------------------------------------------ rotate_geometry
// fftup_rotate_create: the rules and decisions of a rotator (include/fftup.h), arithmetic on the configuration alone.
// The longest line: both shear kernels hold two LDS buffers of two interleaved sequences at that length (rows: R + i G and B + i 0
// side by side; columns: a tile of at least two), 2 * 2 * lpad(4096) * 8 B = 139 280 B of the 160 KB of a gfx950 compute unit.  A
// line of 8192 points would need 278 KB.
static constexpr uint32_t ROTATE_MAX_N = 4096;

int rotate_geometry(const fftup_rotate_config& c, RotateGeometry& G)
{
    const char* who = "fftup_rotate_create: ";
    if (c.precision == 1) return fail(FFTUP_E_UNSUPPORTED_PRECISION, std::string(who) + "precision must be 0 (float planes) or 2 (half planes): there are no -p 1 frames");
    if (c.precision > 2) return fail(FFTUP_E_UNSUPPORTED_PRECISION, std::string(who) + "precision must be 0 (float planes) or 2 (half planes)");
    const uint32_t len[2] = {c.width, c.height};
    for (int a = 0; a < 2; a++) {
        const std::string at = std::string(who) + (a ? "height " : "width ") + std::to_string(len[a]);
        if (len[a] < 2) return fail(FFTUP_E_UNSUPPORTED_SIZE, at + " is below 2");
        if (len[a] > ROTATE_MAX_N) return fail(FFTUP_E_UNSUPPORTED_SIZE, at + " is above " + std::to_string(ROTATE_MAX_N) + " (two LDS buffers of two sequences)");
        if (!is_smooth(len[a])) return fail(FFTUP_E_UNSUPPORTED_SIZE, at + " has a prime factor above 7 (a rotator has no Bluestein path)");
    }
    if (c.max_batch > 64) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "max_batch " + std::to_string(c.max_batch) + " must be <= 64 (0: 4)");
    G.W = c.width; G.H = c.height; G.precision = c.precision;
    G.max_batch = c.max_batch ? c.max_batch : 4;
    G.TK = 2 * c.height <= ROTATE_MAX_N ? 4 : 2;            // the widest tile of 4, 2 whose two buffers fit
    G.lds_x = 2 * sizeof(float2) * (size_t)lpad_size(2 * (int)G.W);
    G.lds_y = 2 * sizeof(float2) * (size_t)lpad_size((int)(G.TK * G.H));
    if (G.lds_x > LDS_GFX950 || G.lds_y > LDS_GFX950) return fail(FFTUP_E_UNSUPPORTED_SIZE, std::string(who) + "the transforms do not fit the LDS");
    return FFTUP_OK;
}

// ------------------------------------------------------------------------------------------------ roll_geometry
// fftup_roll_create: the rules and decisions of a roll estimator (include/fftup.h), arithmetic on the configuration alone.
// The longest window: the transform is zero-padded to twice the window per axis, and 1024 points is the longest line the
// aligner's LDS transforms (which the roll kernels reuse) are sized for.
static constexpr uint32_t ROLL_MAX_WINDOW = 512, ROLL_MIN_WINDOW = 32;

int roll_geometry(const fftup_roll_config& c, RollGeometry& G)
{
    const char* who = "fftup_roll_create: ";
    if (c.width == 0 || c.height == 0) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "width and height must be > 0");
    if (c.width > (1u << 16) || c.height > (1u << 16)) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "width/height above 65536");
    if (c.precision == 1) return fail(FFTUP_E_UNSUPPORTED_PRECISION, std::string(who) + "precision must be 0 (float planes) or 2 (half planes): there are no -p 1 frames");
    if (c.precision > 2) return fail(FFTUP_E_UNSUPPORTED_PRECISION, std::string(who) + "precision must be 0 (float planes) or 2 (half planes)");
    if (c.decimate != 0 && c.decimate != 1 && c.decimate != 2 && c.decimate != 4 && c.decimate != 8)
        return fail(FFTUP_E_INVALID_ARG, std::string(who) + "decimate " + std::to_string(c.decimate) + " must be 1, 2, 4 or 8 (0: automatic)");
    const uint32_t win[2] = {c.window_w, c.window_h};
    for (int a = 0; a < 2; a++)
        if (win[a] && (win[a] < ROLL_MIN_WINDOW || win[a] > ROLL_MAX_WINDOW || (win[a] & (win[a] - 1))))
            return fail(FFTUP_E_INVALID_ARG, std::string(who) + (a ? "window_h " : "window_w ") + std::to_string(win[a]) + " must be a power of two in [32, 512] (0: automatic)");
    if (!(c.band == 0.0f || (c.band > 0.0f && c.band <= 1.0f))) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "band must lie in (0, 1] (0: 0.5)");
    if (c.angles && (c.angles < 32 || c.angles > 1024 || (c.angles & (c.angles - 1))))
        return fail(FFTUP_E_INVALID_ARG, std::string(who) + "angles " + std::to_string(c.angles) + " must be a power of two in [32, 1024] (0: the smaller window length)");
    if (c.upsample && (c.upsample < 4 || c.upsample > 64)) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "upsample " + std::to_string(c.upsample) + " must lie in [4, 64] (0: 32)");
    if (c.max_batch > 65535) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "max_batch must be <= 65535");
    G.W = c.width; G.H = c.height; G.precision = c.precision;
    G.band = c.band == 0.0f ? 0.5f : c.band;
    G.kappa = c.upsample ? c.upsample : 32;
    G.max_batch = c.max_batch ? c.max_batch : 16;
    // automatic d: the smallest whose automatic windows are both at most 512; none: 8, the windows capped
    G.d = c.decimate;
    if (!G.d) {
        G.d = 8;
        for (uint32_t d : {1u, 2u, 4u, 8u})
            if (pow2_floor(c.width / d) <= ROLL_MAX_WINDOW && pow2_floor(c.height / d) <= ROLL_MAX_WINDOW) { G.d = d; break; }
    }
    if (c.width / G.d < ROLL_MIN_WINDOW || c.height / G.d < ROLL_MIN_WINDOW)
        return fail(FFTUP_E_INVALID_ARG, std::string(who) + "a frame of " + std::to_string(c.width) + "x" + std::to_string(c.height) + " has fewer than 32 decimated pixels on an axis (d = " + std::to_string(G.d) + ")");
    G.nx = c.window_w ? c.window_w : std::min(ROLL_MAX_WINDOW, pow2_floor(c.width / G.d));
    G.ny = c.window_h ? c.window_h : std::min(ROLL_MAX_WINDOW, pow2_floor(c.height / G.d));
    if ((uint64_t)G.nx * G.d > c.width) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "window_w * d = " + std::to_string((uint64_t)G.nx * G.d) + " exceeds the frame's width " + std::to_string(c.width));
    if ((uint64_t)G.ny * G.d > c.height) return fail(FFTUP_E_INVALID_ARG, std::string(who) + "window_h * d = " + std::to_string((uint64_t)G.ny * G.d) + " exceeds the frame's height " + std::to_string(c.height));
    G.crop_x = (c.width - G.nx * G.d) / 2;
    G.crop_y = (c.height - G.ny * G.d) / 2;
    G.n = std::min(G.nx, G.ny);
    G.ntheta = c.angles ? c.angles : G.n;
    G.rho_max = (uint32_t)std::floor((double)G.band * (double)G.n);
    G.rho_min = std::max(2u, G.rho_max / 4);
    if (G.rho_max < G.rho_min)
        return fail(FFTUP_E_INVALID_ARG, std::string(who) + "band " + std::to_string(G.band) + " leaves no radius: floor(band * " + std::to_string(G.n) + ") = " + std::to_string(G.rho_max) + " is below 2");
    G.mb = G.ntheta / 4;
    G.K = 2 * G.mb;
    // cx <= n_x and cy <= n_y, the Nyquist bins of the padded transform (band <= 1).  The kernels keep columns -cx - 1 .. cx + 1, which
    // for cx >= n_x - 1 (band = 1) are more than the 2 n_x bins of a row: the definition takes indices modulo the padded length, so
    // column c simply holds bin (c - cx - 1) mod 2 n_x and up to three bins are stored twice, k_x and k_x - 2 n_x alike.  The column
    // kernel pairs column k_x with column -k_x, which are bins k and -k modulo 2 n_x for every k_x up to cx + 1, wrapped or not, so
    // the separation of A and B holds there too.  Rows need no wrap: cy + 1 <= n_y + 1 < 2 n_y.
    G.cx = G.rho_max * (G.nx / G.n);
    G.cy = G.rho_max * (G.ny / G.n);
    return FFTUP_OK;
}
