// fftup_plan.hip -- plan construction behind the C ABI (include/fftup.h): what launchResample() derives from its configuration
// (VkResample.cpp:1409-1617) -- sizes, zero-padding ranges, the R2C rule, factorizations -- device buffers, twiddle tables, the
// plan-time tuner; device enumeration and error text.  The kernels themselves are named in fftup_launch.hip only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_fp16.h>

#include "plan.hpp"
#include "view_tables.hpp"

using namespace fftup;

// ------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

int fail(int code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}

// the marketing name, or -- some driver builds leave it empty -- the architecture name ("gfx950:sramecc+:xnack-")
static const char* device_label(const hipDeviceProp_t& prop) { return prop.name[0] ? prop.name : prop.gcnArchName; }

// ------------------------------------------------------------------------------------------------
static bool is_smooth(uint32_t n)
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
            if (other % (uint32_t)t == 0 && 2 * el * (size_t)lpad_size((int)len * t) <= (size_t)160 * 1024) return t;
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
static StagePlan make_stage_plan(uint32_t n)
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

int dev_alloc(fftup_plan* P, void** ptr, size_t bytes)
{
    hipError_t e = hipMalloc(ptr, bytes);
    if (e != hipSuccess) {
        *ptr = nullptr;
        return fail(FFTUP_E_OUT_OF_MEMORY, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    }
    P->allocs.push_back(*ptr);
    P->device_bytes += bytes;
    return FFTUP_OK;
}

// a table of fp32 pairs computed on the host: device memory owned by the plan, blocking copy
static int upload_table(fftup_plan* P, float2** dptr, const std::vector<float2>& h)
{
    int rc = dev_alloc(P, (void**)dptr, sizeof(float2) * h.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpy(*dptr, h.data(), sizeof(float2) * h.size(), hipMemcpyHostToDevice));
    return FFTUP_OK;
}

static int make_twiddles(fftup_plan* P, float2** dptr, uint32_t n)
{
    if (P->dbl) {                     // double2 table behind the same pointer member
        std::vector<double2> h(n);
        for (uint32_t k = 0; k < n; k++) {
            double a = 2.0 * M_PI * (double)k / (double)n;
            h[k] = make_double2(std::cos(a), std::sin(a));
        }
        int rc = dev_alloc(P, (void**)dptr, sizeof(double2) * n);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(*dptr, h.data(), sizeof(double2) * n, hipMemcpyHostToDevice));
        return FFTUP_OK;
    }
    std::vector<float2> h(n);
    for (uint32_t k = 0; k < n; k++) {
        // exact octant reduction is unnecessary in double; rounded once to fp32
        double a = 2.0 * M_PI * (double)k / (double)n;
        h[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    return upload_table(P, dptr, h);
}

// DCT plans: the pre- and post-rotations exp(i pi k / 2n), k < n, in double, rounded once to fp32 (as make_twiddles)
static int make_rotations(fftup_plan* P, float2** dptr, uint32_t n)
{
    std::vector<float2> h(n);
    for (uint32_t k = 0; k < n; k++) {
        const double a = M_PI * (double)k / (2.0 * (double)n);
        h[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    return upload_table(P, dptr, h);
}

// ---- FFTUP_FLAG_ANY_SIZE: lengths with a prime factor above 7 run as Bluestein transforms (kernels_bluestein.hpp)
static constexpr uint32_t BZ_MAX_N = 4096;      // the longest such length: L = 8192 >= 2 N - 1 always exists and its buffers fit
// do two LDS buffers of `points` complex fp32 points share the 160 KB of a gfx950 compute unit?
static bool two_buffers_fit(size_t points) { return 2 * sizeof(float2) * (size_t)lpad_size((int)points) <= (size_t)160 * 1024; }
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
using fftup_viewtab::host_fft;                   // DFT with exp(+2 pi i nk / n) of a smooth length in double (view_tables.hpp)
// the tables of one Bluestein transform of n points through length L, in double, rounded once to fp32 (as make_twiddles).  The
// phase pi k^2 / n is reduced as (k^2 mod 2n) in 64-bit integers BEFORE the division: it reaches thousands of radians.
static int make_bluestein(fftup_plan* P, BzPlan* z, uint32_t n, uint32_t L, const StagePlan& planL)
{
    std::vector<std::complex<double>> w(n), b(L, std::complex<double>(0.0, 0.0));
    for (uint64_t k = 0; k < n; k++) w[k] = std::polar(1.0, M_PI * (double)((k * k) % (2 * (uint64_t)n)) / (double)n);
    for (uint32_t k = 0; k < n; k++) {
        b[k] = std::conj(w[k]);
        if (k) b[L - k] = std::conj(w[k]);           // (L >= 2n - 1: the two wings do not meet)
    }
    host_fft(b);
    std::vector<float2> hc(n), hb(L);
    for (uint32_t k = 0; k < n; k++) hc[k] = make_float2((float)w[k].real(), (float)w[k].imag());
    for (uint32_t k = 0; k < L; k++) hb[k] = make_float2((float)(b[k].real() / (double)L), (float)(b[k].imag() / (double)L));
    float2 *dc = nullptr, *db = nullptr, *dt = nullptr;
    int rc = dev_alloc(P, (void**)&dc, sizeof(float2) * n);
    if (rc) return rc;
    rc = dev_alloc(P, (void**)&db, sizeof(float2) * L);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dc, hc.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db, hb.data(), sizeof(float2) * L, hipMemcpyHostToDevice));
    rc = make_twiddles(P, &dt, L);
    if (rc) return rc;
    z->L = (int32_t)L; z->plan = planL; z->tw = dt; z->chirp = dc; z->bhat = db;
    return FFTUP_OK;
}

// the sharpen constants reach the reference's shader as "%f" text (VkResample.cpp:893-901, 920)
static float const_via_percent_f(double v, bool half)
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
static bool make_four(const fftup_plan* P, fftup_plan::Four& f, uint32_t n)
{
    f.on = split_four(n, P->csz, &f.n1, &f.n2, &f.tka, &f.tkb);
    if (!f.on) return false;
    f.p1 = make_stage_plan((uint32_t)f.n1); f.p2 = make_stage_plan((uint32_t)f.n2);
    f.ldsA = 2 * P->csz * (size_t)lpad_size(f.n1 * f.tka); f.ldsB = 2 * P->csz * (size_t)lpad_size(f.n2 * f.tkb);
    const int tmax = kernels_generic_max_threads(P->dbl);
    f.thrA = fft_threads(f.n1 * f.tka, tmax); f.thrB = fft_threads(f.n2 * f.tkb, tmax);
    return true;
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
static int jit_factor(float upscale, uint32_t W, uint32_t H, uint32_t uW, uint32_t uH, int zly, int zry, int* DD)
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
static void tune_fused(fftup_plan* P);

// HIP streams ("lanes") the frames of a plan alternate on
int lane_count()
{
    int nl = 3;
    if (const char* e = getenv("FFTUP_STREAMS")) nl = atoi(e);
    return std::max(1, std::min(nl, 4));
}
// Do consecutive frames of this plan overlap on several streams?  A ring of slots (fftup_execute_ring, fftup_submit_rgb8) or
// FFTUP_FLAG_OVERLAP_ITERATIONS (fftup_execute's extension) -- as long as there is more than one stream.
static bool frames_overlap(const fftup_plan* P)
{
    return lane_count() > 1 && (P->ring > 1 || (P->cfg.flags & FFTUP_FLAG_OVERLAP_ITERATIONS));
}
// what the tuner's findings are filed under: the device and whether consecutive frames overlap (what fits beside a strip
// decides) or run one after the other (the kernel's own time decides)
static std::string wisdom_device_key(const fftup_plan* P)
{
    return std::string(P->prop.gcnArchName) + (frames_overlap(P) ? " overlapped" : " sequential");
}

// Row pairs per workgroup (strip) of the fused C2R+sharpen kernel -- a property of the PLAN (results depend on the cuts in
// their last bits, tests/test_gpu_parity.py: test_fused_output_independent_of_strip_length), chosen by how its frames run.
// Frames that overlap on several streams: ONE strip per compute unit -- the rest of every unit is left to the row and column
// kernels of the frames on the other streams, and the frame time is what counts.
// Frames that run one after the other (a plan without a ring: fftup_execute's ordered iterations, the CLI's -n N):
// nothing runs beside a strip, and a workgroup of at most 512 threads (one or two waves per SIMD) does not hide its own
// latencies: two strips per unit (1080p 100 -> 91 us per iteration, 1000x1000 75 -> 62, 2048x1024 77.2 -> 76.0, -p 2
// 82.7 -> 79.7; 768 and 1024 threads: 2-7 % slower with two; profiles/r04_s_strips_per_unit_sequential.txt).
// How many workgroups are resident is the hardware's business.
void set_strip_length(fftup_plan* P)
{
    const int fused_threads = P->tuned ? (int)P->uW / 8 : P->mixed == 3 ? P->jit->choice.fused_t : 256;
    int per_cu = (!frames_overlap(P) && fused_threads <= 512) ? 2 : 1;
    if (const char* e = fftup_jit::experiment("g_per_cu")) per_cu = std::max(1, std::min(4, atoi(e)));
    const int total_pairs = 3 * (int)P->uH / 2, slots = std::max(1, P->prop.multiProcessorCount) * per_cu;
    P->pairs_per_strip = std::max(2, (total_pairs + slots - 1) / slots);
    if (P->u8out) {
        // fused 8-bit store: strips per plane, the three planes' strips of the same rows on ONE of the 8 XCDs (fused_grid):
        // whole triples per XCD, or one compute unit of an XCD gets two strips and the launch takes twice as long
        const int per_xcd = std::max(3, slots / 8) / 3, ppp = (int)P->uH / 2;
        P->pairs_per_strip = std::max(2, (ppp + 8 * per_xcd - 1) / (8 * per_xcd));
    }
    if (const char* e = fftup_jit::experiment("pairs_per_strip")) P->pairs_per_strip = std::max(1, atoi(e));
}
static bool jit_tune_enabled()
{
    const char* e = fftup_jit::experiment("jit_tune");
    return e && atoi(e) != 0;
}

static std::vector<int> stage_radices(const StagePlan& p)
{
    std::vector<int> r;
    for (int s = 0; s < p.nstages; s++) r.push_back(p.radix[s]);
    return r;
}

// ------------------------------------------------------------------------------------------------
extern "C" {

int fftup_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int fftup_device_name(int device, char* buf, size_t buflen)
{
    if (!buf || buflen == 0) return fail(FFTUP_E_INVALID_ARG, "null buffer");
    hipDeviceProp_t prop;
    if (device < 0 || device >= fftup_device_count()) return fail(FFTUP_E_NO_DEVICE, "bad device id");
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    snprintf(buf, buflen, "%s", device_label(prop));
    return FFTUP_OK;
}

int fftup_device_pci_bus_id(int device, char* buf, size_t buflen)
{
    if (!buf || buflen < 16) return fail(FFTUP_E_INVALID_ARG, "buffer of at least 16 bytes needed");
    if (device < 0 || device >= fftup_device_count()) return fail(FFTUP_E_NO_DEVICE, "bad device id");
    HIP_TRY(hipDeviceGetPCIBusId(buf, (int)buflen, device));
    return FFTUP_OK;
}

int fftup_jit_check(uint32_t width, uint32_t height, float upscale, uint32_t precision, const char* arch, char* desc, size_t desclen)
{
    if (desc && desclen) desc[0] = 0;
    if (precision != 0 && precision != 2) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "run-time specialised plans exist for -p 0 and -p 2");
    if (width < 2 || height < 2 || (width & 1) || (height & 1) || width > 65536 || height > 65536 || !is_smooth(width) || !is_smooth(height))
        return fail(FFTUP_E_UNSUPPORTED_SIZE, "sizes must be even and factor into 2,3,5,7");
    fftup_jit::Choice ch;
    if (!(upscale >= 1.0f && upscale <= 8.0f)) return fail(FFTUP_E_INVALID_ARG, "upscale out of range");
    const uint32_t uW = (uint32_t)(upscale * (float)width), uH = (uint32_t)(upscale * (float)height);
    int DD = 1;
    const int D = (uW & 1) || (uH & 1) || !is_smooth(uW) || !is_smooth(uH) || uW > 8192 ? 0 :
                  jit_factor(upscale, width, height, uW, uH, (int)(uint32_t)((float)uH / (2 * upscale)), (int)(uint32_t)((2 * upscale - 1) * (float)uH / (2 * upscale)), &DD);
    if (!D || !fftup_jit::choose((int)width, (int)height, D, precision == 2, stage_radices(make_stage_plan(uW)), ch, "", true, DD))
        return fail(FFTUP_E_UNSUPPORTED_SIZE, "no specialised factorization for this size: the size-generic kernels run it");
    if (desc && desclen) snprintf(desc, desclen, "%s", fftup_jit::describe(ch).c_str());
    if (arch && !*arch) return FFTUP_OK;                     // "": the factorizations only, nothing is compiled
    fftup_jit::Binary bin[2];
    std::string err;
    if (!fftup_jit::compile_both(ch, arch ? arch : "gfx950", bin, err)) return fail(FFTUP_E_HIP, err);
    return FFTUP_OK;
}

void fftup_plan_destroy(fftup_plan* P)
{
    if (!P) return;
    (void)hipSetDevice(P->device);
    if (P->stream) (void)hipStreamSynchronize(P->stream);
    for (size_t l = 1; l < P->lanes.size(); l++) {
        if (P->lanes[l].stream) { (void)hipStreamSynchronize(P->lanes[l].stream); (void)hipStreamDestroy(P->lanes[l].stream); }
        if (P->lanes[l].done) (void)hipEventDestroy(P->lanes[l].done);
    }
    for (auto& qs : P->q) {
        if (qs.done) (void)hipEventDestroy(qs.done);
        if (qs.png.copied) (void)hipEventDestroy(qs.png.copied);
        if (qs.png.meta_host) (void)hipHostFree(qs.png.meta_host);
        if (qs.png.parts_host) (void)hipHostFree(qs.png.parts_host);
    }
    if (P->png_copy) (void)hipStreamDestroy(P->png_copy);
    if (P->dio.start) (void)hipEventDestroy(P->dio.start);
    for (hipEvent_t e : P->dio.done) if (e) (void)hipEventDestroy(e);
    for (void* p : P->allocs) (void)hipFree(p);
    delete P->jit;
    if (P->ev0) (void)hipEventDestroy(P->ev0);
    if (P->ev1) (void)hipEventDestroy(P->ev1);
    if (P->stream) (void)hipStreamDestroy(P->stream);
    delete P;
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

// Centre alignment of one axis N -> M (kernels_odd.hpp): ph[k] = exp(-2 pi i k d / N), d = (N/M - 1)/2, k = 0 .. min(N, M)/2, in
// double, rounded once to fp32 (as make_twiddles).  The phase is -pi k (N - M) / (M N): k (N - M) is reduced modulo 2 M N in
// 64-bit integers BEFORE the division, as the chirp tables' (it reaches hundreds of radians).  M == N: no table (d = 0).
static int make_phases(fftup_plan* P, float2** dptr, uint32_t N, uint32_t M)
{
    *dptr = nullptr;
    if (N == M) return FFTUP_OK;
    const uint32_t n = std::min(N, M) / 2 + 1;
    const int64_t period = 2 * (int64_t)M * (int64_t)N;
    std::vector<float2> h(n);
    for (uint32_t k = 0; k < n; k++) {
        int64_t r = ((int64_t)k * ((int64_t)N - (int64_t)M)) % period;         // in (-period, period)
        if (r > period / 2) r -= period;
        if (r < -period / 2) r += period;
        const double a = -M_PI * (double)r / ((double)M * (double)N);
        h[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    return upload_table(P, dptr, h);
}

// ---- fftup_plan_create_view (kernels_view.hpp, view_tables.hpp)
// the rules of one view, shared by plan creation and fftup_plan_set_view (arithmetic only)
static int check_view(const char* who, const fftup_view* v, uint32_t uW, uint32_t uH)
{
    if (!std::isfinite(v->origin_x) || !std::isfinite(v->origin_y) || !std::isfinite(v->span_x) || !std::isfinite(v->span_y))
        return fail(FFTUP_E_INVALID_ARG, std::string(who) + ": origin and span must be finite numbers");
    const double sx = v->span_x / (double)uW, sy = v->span_y / (double)uH;
    if (!(sx >= 1.0 / 64 && sx <= 8.0)) return fail(FFTUP_E_INVALID_ARG, std::string(who) + ": the step span_x / out_width must lie in [1/64, 8]");
    if (!(sy >= 1.0 / 64 && sy <= 8.0)) return fail(FFTUP_E_INVALID_ARG, std::string(who) + ": the step span_y / out_height must lie in [1/64, 8]");
    return FFTUP_OK;
}
// column tile width of a view plan: the widest of 8, 4, 2, 1 at which max(H, its Bluestein length, L_y) * TK fits twice; 0: none
static int view_col_tk(uint32_t H, uint32_t uH)
{
    const uint32_t Ly = fftup_viewtab::conv_length(H, uH);
    for (int tk : {8, 4, 2, 1})
        if (lds_length(H, tk) && two_buffers_fit((size_t)std::max(lds_length(H, tk), Ly) * tk)) return tk;
    return 0;
}
static float view_factor(const fftup_view& v, uint32_t uW, uint32_t uH)
{
    return (float)std::sqrt((double)uW * (double)uH / (v.span_x * v.span_y));
}
// Aim the plan at `v`: kmax per axis, the spectrum columns kept, the sharpen constant, the tables (blocking copies; the caller has
// made sure nothing of the plan is running).  An axis whose span did not change keeps its chirp tables: only `pre` holds the origin.
static int view_apply(fftup_plan* P, const fftup_view& v, bool first)
{
    struct Ax { fftup_plan::ViewAxis* a; uint32_t N, M; double o, sp, sp_old; };
    const Ax ax[2] = {{&P->vx, P->W, P->uW, v.origin_x, v.span_x, P->vw.span_x}, {&P->vy, P->H, P->uH, v.origin_y, v.span_y, P->vw.span_y}};
    for (const Ax& x : ax) {
        fftup_viewtab::AxisTables t;
        const bool chirp = first || x.sp != x.sp_old;
        fftup_viewtab::make_axis(x.N, x.M, x.o, x.sp, x.a->L, t, chirp);
        x.a->kmax = t.kmax;
        HIP_TRY(hipMemcpy(x.a->pre, t.pre.data(), sizeof(float) * t.pre.size(), hipMemcpyHostToDevice));
        if (chirp) {
            HIP_TRY(hipMemcpy(x.a->post, t.post.data(), sizeof(float) * t.post.size(), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(x.a->bhat, t.bhat.data(), sizeof(float) * t.bhat.size(), hipMemcpyHostToDevice));
        }
    }
    P->vw = v;
    P->ncols = P->vx.kmax + 1;
    P->NT = (P->ncols + P->TK - 1) / P->TK;
    P->cfg.upscale = view_factor(v, P->uW, P->uH);
    P->upsq = const_via_percent_f((double)(P->cfg.upscale * P->cfg.upscale), P->half);
    return FFTUP_OK;
}

// fftup_plan_create (size == nullptr: the output size follows from cfg->upscale), fftup_plan_create_size (size = {uW, uH},
// cfg->upscale ignored) and fftup_plan_create_view (size and view)
static int plan_create(fftup_plan** out, const fftup_config* cfg_in, const uint32_t* size, uint32_t align, const fftup_view* view = nullptr)
{
    if (!out || !cfg_in) return fail(FFTUP_E_INVALID_ARG, "null argument");
    *out = nullptr;
    const bool exact = size != nullptr;
    fftup_config cfg_copy = *cfg_in;
    if (exact) {
        // the effective factor u_e = sqrt(uW uH / (W H)) takes the place of cfg->upscale in the sharpen constant (and only there);
        // 1 until the sizes below are known to be valid
        cfg_copy.upscale = 1.0f;
        cfg_copy.flags &= ~(uint32_t)FFTUP_FLAG_DOWNSCALE;       // (implied per axis: accepted, changes nothing)
    }
    const fftup_config* const cfg = &cfg_copy;
    if (cfg->channels != 3) return fail(FFTUP_E_INVALID_ARG, "channels must be 3 (VkResample.cpp:1368)");
    if (cfg->precision > 2) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "precision must be 0 (single), 1 (double) or 2 (half)");
    const uint32_t W = cfg->width, H = cfg->height;
    // the float -> uint32 casts below are undefined for NaN / out-of-range products: bound the inputs first
    // FFTUP_FLAG_DOWNSCALE: factors in [1/8, 1) instead (a factor below 1 without the flag stays an error)
    const bool down = (cfg->flags & FFTUP_FLAG_DOWNSCALE) != 0;
    if (down && !(cfg->upscale >= 0.125f && cfg->upscale < 1.0f)) return fail(FFTUP_E_INVALID_ARG, "FFTUP_FLAG_DOWNSCALE: the factor must lie in [0.125, 1)");
    if (!down && !(cfg->upscale >= 1.0f && cfg->upscale <= 64.0f)) return fail(FFTUP_E_INVALID_ARG, "upscale must be a finite number in [1, 64]");
    if (W > (1u << 16) || H > (1u << 16)) return fail(FFTUP_E_INVALID_ARG, "width/height above 65536");
    if (cfg->ring > 1024) return fail(FFTUP_E_INVALID_ARG, "ring must be <= 1024");
    if (!(cfg->sharpen == cfg->sharpen)) return fail(FFTUP_E_INVALID_ARG, "sharpen is NaN");
    const uint32_t uW = exact ? size[0] : (uint32_t)(cfg->upscale * (float)W);     // VkResample.cpp:1417-1418
    const uint32_t uH = exact ? size[1] : (uint32_t)(cfg->upscale * (float)H);
    if (view) {
        // fftup_plan_create_view: every rule of such a plan, here (arithmetic, before any device access); the blocks of the other
        // plan kinds below do not apply
        if (W < 2 || H < 2 || uW < 2 || uH < 2) return fail(FFTUP_E_INVALID_ARG, "fftup_plan_create_view: every length (width, height, out_width, out_height) must be at least 2");
        if (int rc = check_view("fftup_plan_create_view", view, uW, uH)) return rc;
        if (cfg->precision == 1) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "fftup_plan_create_view plans exist for -p 0 and -p 2");
        if (cfg->flags & FFTUP_FLAG_DCT) return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view covers the FFT mode only (no FFTUP_FLAG_DCT)");
        if (W > 8192u) return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view: rows of at most 8192 points (no non-R2C or four-step path)");
        if (2 * (uint64_t)(W / 2) + uW > 8192u || fftup_viewtab::conv_length(W, uW) > 8192u)
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view: the row convolution length (2,3,5,7-smooth, at least 2 (width/2) + out_width) must be at most 8192");
        for (uint32_t n : {W, H}) {
            if (!is_smooth(n) && !(cfg->flags & FFTUP_FLAG_ANY_SIZE))
                return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view: width and height must factor into 2,3,5,7; FFTUP_FLAG_ANY_SIZE accepts any length up to 4096");
            if (!is_smooth(n) && n > BZ_MAX_N)
                return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_ANY_SIZE: " + std::to_string(n) + " has a prime factor above 7 and is longer than 4096");
        }
        if (2 * (uint64_t)(H / 2) + uH > 16384u || !view_col_tk(H, uH))
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view: the columns must fit the LDS (two buffers of the column convolution length at a tile width of 1)");
        cfg_copy.upscale = view_factor(*view, uW, uH);
    }
    else if (exact) {
        // fftup_plan_create_size: each axis on its own, up, down or equal, either parity (arithmetic on the sizes)
        if (W < 2 || H < 2 || uW < 2 || uH < 2) return fail(FFTUP_E_INVALID_ARG, "fftup_plan_create_size: every length (width, height, out_width, out_height) must be at least 2");
        if (align > FFTUP_ALIGN_CENTRE) return fail(FFTUP_E_INVALID_ARG, "fftup_plan_create_size: align must be FFTUP_ALIGN_CORNER (0) or FFTUP_ALIGN_CENTRE (1)");
        if (8 * (uint64_t)uW < W || uW > 8 * (uint64_t)W) return fail(FFTUP_E_INVALID_ARG, "fftup_plan_create_size: out_width must lie in [width/8, 8 width]");
        if (8 * (uint64_t)uH < H || uH > 8 * (uint64_t)H) return fail(FFTUP_E_INVALID_ARG, "fftup_plan_create_size: out_height must lie in [height/8, 8 height]");
        cfg_copy.upscale = (float)std::sqrt((double)uW * (double)uH / ((double)W * (double)H));
    }
    // FFTUP_FLAG_ODD_SIZE: odd lengths are valid; `odd`: this plan has one (exact trigonometric resampling, kernels_odd.hpp).  A
    // plan whose four lengths are even is the same plan with or without the flag.
    const bool odd_len = (W & 1) || (H & 1) || (uW & 1) || (uH & 1);
    // (fftup_plan_create_size: always that rule, whatever the parities, FFTUP_FLAG_ODD_SIZE implied)
    const bool odd = exact || (odd_len && (cfg->flags & FFTUP_FLAG_ODD_SIZE));
    if (!exact && (W < 2 || H < 2 || uW < 2 || uH < 2 || (odd_len && !odd) || (!down && (uW < W || uH < H))))
        return fail(FFTUP_E_INVALID_ARG, "width/height (and upscaled sizes) must be even, upscale >= 1; FFTUP_FLAG_ODD_SIZE accepts odd lengths");
    if (down && (uW < 2 || uH < 2 || uW >= W || uH >= H))
        return fail(FFTUP_E_INVALID_ARG, "FFTUP_FLAG_DOWNSCALE: the output sizes must be at least 2 and below the input's");
    // FFTUP_FLAG_ANY_SIZE: lengths with a prime factor above 7 run as Bluestein transforms; `bz`: this plan has one.  A plan
    // whose four lengths are smooth is the same plan with or without the flag.
    // (view plans: only the forward transforms have the input's lengths; the output lengths are the chirp-z transforms' business)
    const bool bz = !is_smooth(W) || !is_smooth(H) || (!view && (!is_smooth(uW) || !is_smooth(uH)));
    if (bz && !(cfg->flags & FFTUP_FLAG_ANY_SIZE))
        return fail(FFTUP_E_UNSUPPORTED_SIZE, "sizes must factor into 2,3,5,7 (vkFFT.h:4719-4726); FFTUP_FLAG_ANY_SIZE accepts any even length up to 4096");
    if (bz && !view) {
        // (arithmetic on the sizes, before any device access)
        if (cfg->flags & FFTUP_FLAG_DCT) return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_DCT plans need sizes that factor into 2,3,5,7 (FFTUP_FLAG_ANY_SIZE covers the FFT modes only)");
        if (cfg->precision == 1) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "FFTUP_FLAG_ANY_SIZE plans with a non-smooth length exist for -p 0 and -p 2");
        for (uint32_t n : {W, H, uW, uH})
            if (!is_smooth(n) && n > BZ_MAX_N)
                return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_ANY_SIZE: " + std::to_string(n) + " has a prime factor above 7 and is longer than 4096");
        // the smooth lengths of such a plan keep their Stockham transforms in the same kernels: two-buffer R2C rows, columns in LDS
        if (W > 8192u || uW > 8192u)
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_ANY_SIZE: a plan with a non-smooth length needs rows of at most 8192 points (no non-R2C or four-step path)");
        if (!bluestein_col_tk(H, uH))
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_ANY_SIZE: a plan with a non-smooth length needs columns that fit the LDS (no four-step columns)");
    }
    if (odd && !exact) {
        // the bounds of Bluestein plans (arithmetic on the sizes, before any device access): two-buffer R2C rows, columns in LDS
        if (cfg->flags & FFTUP_FLAG_DCT) return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_DCT plans need even sizes (FFTUP_FLAG_ODD_SIZE covers the FFT modes only)");
        if (cfg->precision == 1) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "FFTUP_FLAG_ODD_SIZE plans with an odd length exist for -p 0 and -p 2");
        if (W > 8192u || uW > 8192u)
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_ODD_SIZE: a plan with an odd length needs rows of at most 8192 points (no non-R2C or four-step path)");
        if (!bluestein_col_tk(H, uH))
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_ODD_SIZE: a plan with an odd length needs columns that fit the LDS (no four-step columns)");
    }
    if (exact && !view) {
        // the same bounds: these plans run the odd-size plans' kernels
        if (cfg->flags & FFTUP_FLAG_DCT) return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_size covers the FFT mode only (no FFTUP_FLAG_DCT)");
        if (cfg->precision == 1) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "fftup_plan_create_size plans exist for -p 0 and -p 2");
        if (W > 8192u || uW > 8192u)
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_size: rows of at most 8192 points (no non-R2C or four-step path)");
        if (!bluestein_col_tk(H, uH))
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_size: the columns must fit the LDS (no four-step columns)");
    }
    // R2C rule of the reference: uW <= maxComputeSharedMemorySize/8 with 64 KB (VkResample.cpp:1424; complexSizeCalc = 16
    // for -p 1, VkResample.cpp:1334-1336, halves the limit); beyond it the full complex path runs
    const bool cplx = uW > (cfg->precision == 1 ? 4096u : 8192u);
    // DCT plans (FFTUP_FLAG_DCT): fp32 / fp16 storage, rows in one LDS launch (no non-R2C-like path for uW beyond 8192)
    const bool dct = (cfg->flags & FFTUP_FLAG_DCT) != 0;
    if (dct && cfg->precision == 1) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "FFTUP_FLAG_DCT plans exist for -p 0 and -p 2");
    if (dct && uW > 8192u) return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_DCT plans need an upscaled width of at most 8192");
    // downscale plans: the same storage, the input rows in one two-buffer LDS launch (no four-step or non-R2C downscale)
    if (down && cfg->precision == 1) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "FFTUP_FLAG_DOWNSCALE plans exist for -p 0 and -p 2");
    if (down && W > 8192u) return fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_DOWNSCALE plans need an input width of at most 8192");
    // (checked here, before any device access: gfx950 has 160 KB of LDS per workgroup.)  Non-R2C rows whose two Stockham
    // buffers do not fit run in ONE buffer (fft_lds_inplace: up to 16 384 complex fp32 points, 1024 threads, every stage
    // N/R <= (16/R) * 1024: radix 7 up to 14336 points, 3 and 5 up to 15360); the reference switches to multi-upload plans there (vkFFT.h:4773-4992)
    auto rows_fit = [&](uint32_t n) -> int {             // 2: two buffers, 1: one buffer (in place), 0: not at all
        const size_t el = cfg->precision == 1 ? 16 : 8, lds = (size_t)160 * 1024;
        if (2 * el * (size_t)lpad_size((int)n) <= lds) return 2;
        if (cfg->precision == 1 || el * (size_t)lpad_size((int)n) > lds) return 0;
        const StagePlan sp = make_stage_plan(n);
        for (int st = 0; st < sp.nstages; st++)
            if (!stage_fits_inplace((int)n, sp.radix[st], 1024, 16)) return 0;
        return 1;
    };
    // ... and rows beyond one buffer run in four steps through HBM (k_row4_a / k_row4_b), as the reference's multi-upload plans
    {
        int a, b, t, t2;
        const size_t el = cfg->precision == 1 ? 16 : 8;
        if (cplx && ((!rows_fit(uW) && !split_four(uW, el, &a, &b, &t, &t2)) || (!rows_fit(W) && !split_four(W, el, &a, &b, &t, &t2))))
            return fail(FFTUP_E_UNSUPPORTED_SIZE, "row too long: no four-step split of the row length fits the LDS");
    }

    int ndev = fftup_device_count();
    if (ndev <= 0) return fail(FFTUP_E_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(FFTUP_E_NO_DEVICE, "device id out of range");

    fftup_plan* P = new fftup_plan();
    P->cfg = *cfg;
    P->W = W; P->H = H; P->uW = uW; P->uH = uH;
    P->ring = cfg->ring ? cfg->ring : 1;
    P->half = cfg->precision == 2;
    P->dbl = cfg->precision == 1;
    P->cplx = cplx;
    P->dct = dct;
    P->down = down;
    P->bz = bz;
    P->odd = odd;
    P->exact = exact;
    P->align = exact ? align : 0;
    P->view = view != nullptr;
    // (FFT downscale plans keep only the bins the output holds, kx <= uW/2: S1, S2 and the column pass shrink with the output)
    // (odd plans: the bins both lengths hold, kx <= min(W, uW)/2 -- floor: an odd length has (n + 1)/2 bins from 0 up, no Nyquist bin)
    P->ncols = cplx ? (int)W : (down && !dct) ? (int)(uW / 2 + 1) : (int)(W / 2 + 1);
    if (odd) P->ncols = (int)(std::min(W, uW) / 2 + 1);
    if (view) P->ncols = (int)(W / 2 + 1);              // (the worst case: the buffers below hold any view; view_apply sets the current one)
    P->esz = P->dbl ? 8 : (P->half ? 2 : 4);
    P->csz = P->dbl ? 16 : 8;
    P->device = cfg->device;
    int rc = FFTUP_OK;
#define PLAN_TRY(expr)                                                                             \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            rc = fail(FFTUP_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
            goto bad;                                                                              \
        }                                                                                          \
    } while (0)
#define PLAN_RC(expr)                                                                              \
    do {                                                                                           \
        rc = (expr);                                                                               \
        if (rc) goto bad;                                                                          \
    } while (0)

    {
        PLAN_TRY(hipSetDevice(P->device));
        PLAN_TRY(hipGetDeviceProperties(&P->prop, P->device));
        PLAN_TRY(hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking));
        PLAN_TRY(hipEventCreate(&P->ev0));
        PLAN_TRY(hipEventCreate(&P->ev1));

        // zero-padding ranges exactly as launchResample computes them (float math, uint32 store)
        const float u = cfg->upscale;
        P->zlx = (int)(W / 2);
        P->zrx = cplx ? (int)(uint32_t)((2 * u - 1) * (float)uW / (2 * u)) : (int)(uW / 2);      // VR:1498 / VR:1493
        // (downscale plans have no padding: no guard, and 2u - 1 < 0 would make the cast below undefined)
        P->zly = (down || exact) ? 0 : (int)(uint32_t)((float)uH / (2 * u));
        P->zry = (down || exact) ? 0 : (int)(uint32_t)((2 * u - 1) * (float)uH / (2 * u));

        P->planW = make_stage_plan(W);
        P->planH = make_stage_plan(H);
        P->planUW = make_stage_plan(uW);
        P->planUH = make_stage_plan(uH);

        const size_t lds_max = P->prop.sharedMemPerBlock ? P->prop.sharedMemPerBlock : 65536;
        // size-specialised kernels: u == 2 and power-of-two sizes with instantiated plans
        // (experiment aot=0: the sizes with ahead-of-time kernels go through the plan-time compiler as well)
        const char* const aot_e = fftup_jit::experiment("aot");
        const bool aot = !(aot_e && atoi(aot_e) == 0);
        P->tuned = aot && !P->dbl && !cplx && !dct && !down && !exact && !(cfg->flags & FFTUP_FLAG_GENERIC_KERNELS) && uW == 2 * W && uH == 2 * H &&
                   (W == 512 || W == 1024 || W == 2048) && (H == 256 || H == 512 || H == 1024);
        P->TK = 0;
        if (P->tuned) {
            P->TK = TUNED_TK;
            P->ldsCol = kernels_tuned_col_lds(H);
        } else {
            // u = 2 with the symmetric guard: the polyphase column kernel (k_col_poly: forward, phase, length-H inverse in ONE buffer of
            // H TK points, odd rows out; the C2R kernel takes the even rows from S1) where its stages run in place
            const char* const poly_e = fftup_jit::experiment("generic_poly");
            if (!cplx && !dct && !down && !odd && is_smooth(H) && uW == 2 * W && uH == 2 * H && P->zly == (int)(H / 2) && P->zry == (int)(uH - H / 2) && !(poly_e && atoi(poly_e) == 0)) {
                for (int tk : {8, 4, 2, 1}) {
                    const size_t need = P->csz * (size_t)lpad_size((int)H * tk);
                    const int thr = inplace_threads(P->planH, tk, COL_INPLACE_PT, kernels_generic_max_threads(P->dbl));
                    if (thr && need <= lds_max / 2) { P->TK = tk; P->ldsCol = need; P->poly = true; P->thrCol = thr; break; }    // (two workgroups per compute unit)
                }
            }
            // -p 1 R2C plans: ONE buffer where every stage of both column transforms runs in place with COL_INPLACE_PT points per thread (k_col<.., true>)
            if (!P->TK && P->dbl && !cplx) {
                for (int tk : {8, 4, 2, 1}) {
                    const size_t need = P->csz * (size_t)lpad_size((int)uH * tk);
                    const int tmax = kernels_generic_max_threads(true);
                    const int thr = std::max(inplace_threads(P->planH, tk, COL_INPLACE_PT, tmax), inplace_threads(P->planUH, tk, COL_INPLACE_PT, tmax));
                    const bool ok = inplace_threads(P->planH, tk, COL_INPLACE_PT, tmax) && inplace_threads(P->planUH, tk, COL_INPLACE_PT, tmax) &&
                                    need <= lds_max / 2 && (size_t)(H / 2) * tk <= (size_t)COL_INPLACE_PT * thr;  // (two workgroups per compute unit)
                    if (ok) { P->TK = tk; P->ldsCol = need; P->inplaceC = true; P->thrCol = thr; break; }
                }
            }
            // a Bluestein column transform: buffers of L * TK points (bluestein_col_tk: checked before any device access); the
            // column kernel of an odd plan is sized the same way, max(length, L) * TK with L = length for a smooth one
            if (view) {
                P->vx.L = fftup_viewtab::conv_length(W, uW); P->vy.L = fftup_viewtab::conv_length(H, uH);
                P->vx.planL = make_stage_plan(P->vx.L); P->vy.planL = make_stage_plan(P->vy.L);
                P->TK = view_col_tk(H, uH);
                P->ldsCol = 2 * P->csz * (size_t)lpad_size((int)(std::max(lds_length(H, P->TK), P->vy.L) * (uint32_t)P->TK));
                if (P->ldsCol > lds_max) { rc = fail(FFTUP_E_UNSUPPORTED_SIZE, "fftup_plan_create_view: this device's LDS does not hold the column transform"); goto bad; }
            }
            if (!P->TK && (odd || !is_smooth(H) || !is_smooth(uH))) {
                P->TK = bluestein_col_tk(H, uH);
                P->ldsCol = 2 * P->csz * (size_t)lpad_size((int)(std::max(std::max(H, uH), std::max(lds_length(H, P->TK), lds_length(uH, P->TK))) * (uint32_t)P->TK));
                if (P->ldsCol > lds_max) { rc = fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_ANY_SIZE: this device's LDS does not hold the column transform"); goto bad; }
            }
            // column tile width: widest of 8,4,2,1 whose ping-pong buffers fit in LDS (downscale plans: the forward transform,
            // length H, is the longer one)
            if (!P->TK) for (int tk : {8, 4, 2, 1}) {
                size_t need = 2 * P->csz * (size_t)lpad_size((int)std::max(H, uH) * tk);
                if (need <= lds_max) { P->TK = tk; P->ldsCol = need; break; }
            }
        }
        if (!P->TK && dct) { rc = fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_DCT: the columns do not fit the LDS (no four-step DCT)"); goto bad; }
        if (!P->TK && down) { rc = fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_DOWNSCALE: the columns do not fit the LDS (no four-step downscale)"); goto bad; }
        if (!P->TK) {
            // not even one column fits: tiles of one column, both column transforms in four steps through HBM (k_row4_a / k_row4_b)
            P->TK = 1; P->ldsCol = 0;
            if (!make_four(P, P->colF, H) || !make_four(P, P->colI, uH)) {
                rc = fail(FFTUP_E_UNSUPPORTED_SIZE, "column too long: no four-step split of the height fits the LDS"); goto bad;
            }
        }
        if (aot && !P->dbl && !cplx && !dct && !down && !exact && !P->tuned && !(cfg->flags & FFTUP_FLAG_GENERIC_KERNELS) && uW == 2 * W && uH == 2 * H && P->TK >= 4) {
            P->mixed = kernels_aot_mixed_plan(W, H);                    // 1920x1080, 1280x720
        }
        if (P->mixed) { P->TK = 4; P->ldsCol = sizeof(float2) * (size_t)H * 4; }             // k_col_m: one in-place buffer
        // any other size with an integer or half-integer upscale factor: kernels specialised for it now (the counterpart
        // of VkFFT generating its shaders at plan time)
        if (!P->dbl && !cplx && !dct && !down && !bz && !odd && !P->tuned && !P->mixed && !(cfg->flags & (FFTUP_FLAG_GENERIC_KERNELS | FFTUP_FLAG_UNFUSED_SHARPEN)) && jit_enabled()) {
            int DD = 1;
            const int D = jit_factor(cfg->upscale, W, H, uW, uH, P->zly, P->zry, &DD);
            if (D) {
                fftup_jit::Choice ch;
                std::string jerr;
                if (fftup_jit::choose((int)W, (int)H, D, P->half, stage_radices(P->planUW), ch, wisdom_device_key(P), true, DD)) {
                    ch.u8out = (cfg->flags & FFTUP_FLAG_FUSE_U8_STORE) != 0;         // (such a plan is always fused)
                    P->jit = fftup_jit::load(ch, P->prop.gcnArchName, jerr);
                    if (P->jit) {
                        P->mixed = 3; P->U = ch.U; P->TK = 4; P->ldsCol = P->jit->choice.col_lds;
                        // (inputs taller than 4800 rows: the size-generic plan above would have run its columns in four steps through
                        // HBM -- the specialised column kernel holds two whole columns in LDS instead)
                        P->colF = fftup_plan::Four{}; P->colI = fftup_plan::Four{};
                    }
                    else if (getenv("FFTUP_JIT_VERBOSE")) fprintf(stderr, "fftup: run-time specialisation failed, size-generic kernels in use: %s\n", jerr.c_str());
                }
            }
        }
        if (P->tuned || P->mixed) P->poly = false;               // (their own column kernels)
        // The family, decided here once.  The rules above make the families exclusive wherever two of them could claim a plan (the
        // long rows of cplx and the double arithmetic of f64 exist in the size-generic upscale kernels only; the ahead-of-time and
        // plan-time kernels take none of the other modes): stated here, so that no order of tests has to be relied on.  Three
        // pairs are no conflict: view plans are `odd` and `exact` (they run the odd plans' row kernel), odd plans may be `down`
        // (the direction is a parameter of their kernels), DCT plans may be `down` too.
        if ((cplx && (dct || down || odd || view || bz)) || (P->dbl && (dct || down || odd || view || bz)) || (dct && (odd || view || bz)) ||
            ((P->tuned || P->mixed) && (cplx || P->dbl || dct || down || odd || view || bz)) || (P->tuned && P->mixed)) {
            rc = fail(FFTUP_E_INVALID_ARG, "internal: the plan rules let two kernel families claim this plan"); goto bad;
        }
        using Family = fftup_plan::Family;
        P->family = cplx ? Family::cplx : P->dbl ? Family::f64 : dct ? Family::dct : view ? Family::view : odd ? Family::odd : down ? Family::down
                    : P->tuned ? Family::tuned : P->mixed == 3 ? Family::mixed_jit : P->mixed ? Family::mixed_aot : Family::generic;
        P->fused = (P->tuned || P->mixed) && !(cfg->flags & FFTUP_FLAG_UNFUSED_SHARPEN);
        P->u8out = P->fused && (cfg->flags & FFTUP_FLAG_FUSE_U8_STORE);
        set_strip_length(P);
        P->NT = (P->ncols + P->TK - 1) / P->TK;
        P->ldsRowF = 2 * P->csz * (size_t)lpad_size((int)W);
        P->ldsRowI = 2 * P->csz * (size_t)lpad_size((int)uW);
        if (bz) {                                            // Bluestein rows: buffers of L points
            P->ldsRowF = 2 * P->csz * (size_t)lpad_size((int)lds_length(W, 1));
            P->ldsRowI = 2 * P->csz * (size_t)lpad_size((int)lds_length(uW, 1));
            if (P->ldsRowF > lds_max) { rc = fail(FFTUP_E_UNSUPPORTED_SIZE, "FFTUP_FLAG_ANY_SIZE: this device's LDS does not hold the row transform"); goto bad; }
        }
        if (cplx) {                                          // long non-R2C rows: one buffer, in place (rows_fit above)
            P->inplaceF = rows_fit(W) == 1; P->inplaceI = rows_fit(uW) == 1;
            if (P->inplaceF) P->ldsRowF /= 2;
            if (P->inplaceI) P->ldsRowI /= 2;
            // ... or four steps through HBM (a split exists: checked before any device access)
            if (!rows_fit(W)) { make_four(P, P->fourF, W); P->ldsRowF = 0; }
            if (!rows_fit(uW)) { make_four(P, P->fourI, uW); P->ldsRowI = 0; }
        }
        if (view) P->ldsRowI = 2 * P->csz * (size_t)lpad_size((int)P->vx.L);      // (L_x >= out_width)
        if (P->ldsRowI > lds_max) { rc = fail(FFTUP_E_UNSUPPORTED_SIZE, "upscaled width too large for LDS"); goto bad; }
        {
            const int tmax = kernels_generic_max_threads(P->dbl);
            P->thrW = fft_threads((int)W, tmax);
            P->thrUW = fft_threads((int)uW, tmax);
            if (!(P->poly || P->inplaceC)) P->thrCol = fft_threads((int)std::max(H, uH) * P->TK, tmax);     // (in-place column plans chose theirs above)
            if (bz) {                                        // the sequences in LDS are the Bluestein transforms'
                P->thrW = fft_threads((int)lds_length(W, 1), tmax);
                P->thrUW = fft_threads((int)lds_length(uW, 1), tmax);
                if (!P->poly) P->thrCol = fft_threads((int)std::max(lds_length(H, P->TK), lds_length(uH, P->TK)) * P->TK, tmax);
            }
            if (view) {                                      // the chirp-z transforms: the sequences hold L points
                P->thrUW = fft_threads((int)P->vx.L, tmax);
                P->thrCol = fft_threads((int)std::max(lds_length(H, P->TK), P->vy.L) * P->TK, tmax);
            }
            // -p 1 R2C rows: one LDS buffer where every stage runs in place with 8 points per thread (two workgroups per compute unit)
            if (P->dbl && !cplx) {
                const int tf = inplace_threads(P->planW, 1, 8, tmax), ti = inplace_threads(P->planUW, 1, 8, tmax);
                if (tf) { P->inplaceF = true; P->thrW = tf; P->ldsRowF /= 2; }
                if (ti) { P->inplaceI = true; P->thrUW = ti; P->ldsRowI /= 2; }
            }
        }

        P->upsq = const_via_percent_f((double)(cfg->upscale * cfg->upscale), P->half);   // VkResample.cpp:1615
        P->coef = const_via_percent_f((double)cfg->sharpen, P->half);                    // VkResample.cpp:1616

        PLAN_RC(make_twiddles(P, &P->twW, W));
        PLAN_RC(make_twiddles(P, &P->twH, H));
        PLAN_RC(make_twiddles(P, &P->twUW, uW));
        PLAN_RC(make_twiddles(P, &P->twUH, uH));
        for (fftup_plan::Four* f : {&P->fourF, &P->fourI, &P->colF, &P->colI})
            if (f->on) { PLAN_RC(make_twiddles(P, &f->tw1, (uint32_t)f->n1)); PLAN_RC(make_twiddles(P, &f->tw2, (uint32_t)f->n2)); }
        if (bz) {
            const std::pair<BzPlan*, uint32_t> axes[4] = {{&P->bzW, W}, {&P->bzH, H}, {&P->bzUW, uW}, {&P->bzUH, uH}};
            for (int i = 0; i < 4; i++)
                if (!is_smooth(axes[i].second) && !(view && i >= 2)) {
                    const uint32_t L = lds_length(axes[i].second, (i & 1) ? P->TK : 1);
                    PLAN_RC(make_bluestein(P, axes[i].first, axes[i].second, L, make_stage_plan(L)));
                }
        }
        if (exact && align == FFTUP_ALIGN_CENTRE) {
            PLAN_RC(make_phases(P, &P->phW, W, uW));
            PLAN_RC(make_phases(P, &P->phH, H, uH));
        }
        if (view) {
            // tables of the worst case: 2 (N/2) + 1 bins in, M points out, L points of the convolution
            const std::pair<fftup_plan::ViewAxis*, std::pair<uint32_t, uint32_t>> vaxes[2] = {{&P->vx, {W, uW}}, {&P->vy, {H, uH}}};
            for (auto& va : vaxes) {
                PLAN_RC(make_twiddles(P, &va.first->tw, va.first->L));
                PLAN_RC(dev_alloc(P, (void**)&va.first->pre, sizeof(float2) * (2 * (size_t)(va.second.first / 2) + 1)));
                PLAN_RC(dev_alloc(P, (void**)&va.first->post, sizeof(float2) * va.second.second));
                PLAN_RC(dev_alloc(P, (void**)&va.first->bhat, sizeof(float2) * va.first->L));
            }
        }
        if (dct) {
            PLAN_RC(make_rotations(P, &P->rotW, W));
            PLAN_RC(make_rotations(P, &P->rotH, H));
            PLAN_RC(make_rotations(P, &P->rotUW, uW));
            PLAN_RC(make_rotations(P, &P->rotUH, uH));
        }

        const size_t esz = P->esz;
        P->in_plane_stride = (size_t)(W + 2) * H;                    // VkResample.cpp:1644
        P->in_planar.assign(P->ring, nullptr);
        P->in_u8.assign(P->ring, nullptr);
        P->in_kind.assign(P->ring, 0);
        P->out.assign(P->ring, nullptr);
        for (uint32_t s = 0; s < P->ring; s++) {
            PLAN_RC(dev_alloc(P, &P->in_planar[s], 3 * P->in_plane_stride * esz));
            PLAN_RC(dev_alloc(P, (void**)&P->in_u8[s], (size_t)3 * W * H));
            PLAN_RC(dev_alloc(P, &P->out[s], (size_t)3 * uW * uH * (P->u8out ? 1 : esz) + 8));          // (+ 8: readers of whole words)
        }
        // tuned plans (k_col_t): S2 holds the odd rows only and sits right behind S1 in ONE allocation (the fused
        // kernel addresses both with 32-bit offsets from one base)
        const size_t s1_elems = (size_t)3 * P->NT * H * P->TK;
        auto alloc_spectra = [&](float2** s1, float2** s2) -> int {
            if ((P->tuned || P->mixed) && P->U >= 2) {
                int r = dev_alloc(P, (void**)s1, P->csz * (size_t)P->U * s1_elems);       // S1 + the U-1 residue buffers
                *s2 = r ? nullptr : *s1 + s1_elems;
                return r;
            }
            int r = dev_alloc(P, (void**)s1, P->csz * s1_elems);
            return r ? r : dev_alloc(P, (void**)s2, P->csz * 3 * (size_t)P->NT * uH * P->TK);
        };
        PLAN_RC(alloc_spectra(&P->S1, &P->S2));
        // the pre-sharpen image (the reference's tempBuffer): every frame of an unfused plan goes through it; a fused plan
        // only needs one for the fftup_download_presharpen tap, which allocates it on first use (ensure_R)
        P->r_bytes = (size_t)3 * uW * uH * (cplx ? (P->half ? 4 : P->csz) : esz);  // non-R2C path: complex pre-sharpen image (binary16 pairs for -p 2)
        if (!P->fused) PLAN_RC(dev_alloc(P, &P->R, P->r_bytes));
        if (!P->u8out) PLAN_RC(dev_alloc(P, (void**)&P->out_u8, (size_t)3 * uW * uH + 8));   // staging of the conversion launch (+ 8: k_png_filter reads whole words)
        {
            P->nlanes = lane_count();
            P->lanes.resize(P->nlanes);
            P->lanes[0].stream = P->stream; P->lanes[0].S1 = P->S1; P->lanes[0].S2 = P->S2; P->lanes[0].R = P->R;
            const size_t t4_bytes = P->csz * 3 * std::max(std::max(P->fourF.on ? (size_t)W * H : 0, P->fourI.on ? (size_t)uW * uH : 0),
                                                          P->colI.on ? (size_t)P->ncols * uH : 0);
            if (t4_bytes) PLAN_RC(dev_alloc(P, &P->lanes[0].T4, t4_bytes));
            for (int l = 1; l < P->nlanes; l++) {
                PLAN_TRY(hipStreamCreateWithFlags(&P->lanes[l].stream, hipStreamNonBlocking));
                PLAN_TRY(hipEventCreateWithFlags(&P->lanes[l].done, hipEventDisableTiming));
                PLAN_RC(alloc_spectra(&P->lanes[l].S1, &P->lanes[l].S2));
                if (!P->fused) PLAN_RC(dev_alloc(P, &P->lanes[l].R, P->r_bytes));
                if (t4_bytes) PLAN_RC(dev_alloc(P, &P->lanes[l].T4, t4_bytes));
            }
        }
        if (view) PLAN_RC(view_apply(P, *view, true));       // (after the allocations above: they are the worst case's)
        PLAN_RC(kernels_set_attributes(P));          // dynamic LDS above 64 KB for the kernels THIS plan launches (fftup_launch.hip)
        if (P->mixed == 3 && ((cfg->flags & FFTUP_FLAG_TUNE_PLAN) || jit_tune_enabled())) tune_fused(P);
    }
    png_geometry(P);                       // (fixed per plan: fftup_png_bound may be asked by several threads at once)
    *out = P;
    return FFTUP_OK;
bad:
    fftup_plan_destroy(P);
    return rc;
#undef PLAN_TRY
#undef PLAN_RC
}

int fftup_plan_create(fftup_plan** out, const fftup_config* cfg) { return plan_create(out, cfg, nullptr, 0); }

int fftup_plan_create_size(fftup_plan** out, const fftup_config* cfg, uint32_t out_width, uint32_t out_height, uint32_t align)
{
    const uint32_t size[2] = {out_width, out_height};
    return plan_create(out, cfg, size, align);
}

int fftup_plan_create_view(fftup_plan** out, const fftup_config* cfg, uint32_t out_width, uint32_t out_height, const fftup_view* view)
{
    if (out) *out = nullptr;
    if (!out || !cfg || !view) return fail(FFTUP_E_INVALID_ARG, "null argument");
    const uint32_t size[2] = {out_width, out_height};
    return plan_create(out, cfg, size, FFTUP_ALIGN_CORNER, view);
}

int fftup_plan_set_view(fftup_plan* P, const fftup_view* view)
{
    if (!P || !view) return fail(FFTUP_E_INVALID_ARG, "null argument");
    if (!P->view) return fail(FFTUP_E_INVALID_ARG, "fftup_plan_set_view: not a view plan (fftup_plan_create_view makes one)");
    if (int rc = check_view("fftup_plan_set_view", view, P->uW, P->uH)) return rc;
    HIP_TRY(hipSetDevice(P->device));
    // the tables are read by the kernels of frames in flight: wait for the plan's own streams first
    for (auto& lane : P->lanes) HIP_TRY(hipStreamSynchronize(lane.stream));
    return view_apply(P, *view, false);
}

int fftup_plan_describe(const fftup_plan* P, char* buf, size_t buflen)
{
    if (!P || !buf || !buflen) return fail(FFTUP_E_INVALID_ARG, "null argument");
    std::string s;
    using Family = fftup_plan::Family;
    const std::string half = P->half ? ", half storage" : "", tiles = std::to_string(P->TK);
    // (odd, exact and view plans)
    const std::string resampled = " (size-generic kernels, " + std::to_string(P->ncols) + " spectrum columns, LDS ping-pong, run-time radix lists, column tiles of " + tiles + ")" + half;
    const std::string rows_cols = ", rows " + std::to_string(P->W) + "->" + std::to_string(P->uW) + ", columns " + std::to_string(P->H) + "->" + std::to_string(P->uH);
    switch (P->family) {
    case Family::dct:
        s = std::string(P->down ? "downscale: dct: size-generic DCT-II / truncate / DCT-III kernels" : "dct: size-generic DCT-II / zero-pad / DCT-III kernels")
            + " (LDS ping-pong, run-time radix lists, column tiles of " + tiles + " column pairs)" + half;
        break;
    case Family::view: {
        char t[256];
        snprintf(t, sizeof t, "view: chirp-z resampling, rows %u->%u origin %.17g span %.17g (kmax %d, L=%u), columns %u->%u origin %.17g span %.17g (kmax %d, L=%u)",
                 P->W, P->uW, P->vw.origin_x, P->vw.span_x, P->vx.kmax, P->vx.L, P->H, P->uH, P->vw.origin_y, P->vw.span_y, P->vy.kmax, P->vy.L);
        s = t + resampled;
        break;
    }
    case Family::odd:
        if (P->exact) s = "exact size: exact trigonometric resampling" + rows_cols + (P->align == FFTUP_ALIGN_CENTRE ? ", pixel centres aligned" : ", pixel 0 on pixel 0") + resampled;
        else s = std::string(P->down ? "downscale: " : "") + "odd sizes: exact trigonometric resampling" + rows_cols + resampled;
        break;
    case Family::down:
        s = "downscale: size-generic kernels, spectrum cropped to " + std::to_string(P->ncols) + " columns at the row stage (LDS ping-pong, "
            "run-time radix lists, column tiles of " + tiles + ")" + half;
        break;
    case Family::mixed_jit: s = "specialised at plan time: " + fftup_jit::describe(P->jit->choice); break;
    case Family::tuned:
        s = "ahead-of-time power-of-two kernels (radix 8, 8 points per thread; fused C2R+sharpen " + std::string(P->fused ? "on" : "off") + ")"
            + "; column kernel with digit-swap exchanges";
        break;
    case Family::mixed_aot:
        s = std::string("ahead-of-time mixed-radix kernels: ") + (P->mixed == 1 ? "row 15*8*16, col 9*10*12, fused 16*16*15" : "row 5*16*16, col 9*8*10, fused 16*16*10");
        break;
    case Family::cplx: s = "size-generic kernels, non-R2C path (full complex transforms)"; break;
    case Family::generic: case Family::f64:
        s = std::string("size-generic kernels (") + ((P->inplaceF || P->inplaceI || P->inplaceC) ? "in place in one LDS buffer" : "LDS ping-pong") + ", run-time radix lists"
            + (P->poly ? ", polyphase column pass)" : ")")
            + (P->dbl ? ", double" : "");
        break;
    }
    auto four = [&](const char* what, const fftup_plan::Four& f) {
        if (f.on) s += std::string("; ") + what + " in four steps " + std::to_string(f.n1) + "*" + std::to_string(f.n2) + " (tiles of " + std::to_string(f.tka) + " / " + std::to_string(f.tkb) + ")";
    };
    four("forward rows", P->fourF); four("inverse rows", P->fourI); four("forward columns", P->colF); four("inverse columns", P->colI);
    if (P->bz && P->family == Family::view) {
        if (P->bzW.L) s += "; forward rows bluestein L=" + std::to_string(P->bzW.L);
        if (P->bzH.L) s += "; forward columns bluestein L=" + std::to_string(P->bzH.L);
    }
    else if (P->bz) {
        // the Bluestein axes and their lengths L (forward / inverse; "-": that transform is a direct one)
        auto axis = [&](const char* what, uint32_t n, uint32_t un, const BzPlan& f, const BzPlan& i) {
            if (!f.L && !i.L) return;
            s += std::string("; ") + what + " " + std::to_string(n) + "->" + std::to_string(un) + " bluestein L=" + (f.L ? std::to_string(f.L) : std::string("-")) + "/"
                 + (i.L ? std::to_string(i.L) : std::string("-"));
        };
        axis("rows", P->W, P->uW, P->bzW, P->bzUW);
        axis("columns", P->H, P->uH, P->bzH, P->bzUH);
        s += "; column tiles of " + std::to_string(P->TK);
    }
    if (P->u8out) s += "; fused 8-bit RGB store";
    snprintf(buf, buflen, "%s", s.c_str());
    return FFTUP_OK;
}

int fftup_plan_info(const fftup_plan* P, fftup_info* info)
{
    if (!P || !info) return fail(FFTUP_E_INVALID_ARG, "null argument");
    memset(info, 0, sizeof *info);
    info->out_width = P->uW;
    info->out_height = P->uH;
    info->num_kernels = P->fused ? 3 : 4;
    info->tuned = P->mixed == 3 ? 2 : ((P->tuned || P->mixed) ? 1 : 0);
    // B_alg = in + 2*S1 + 2*S2 + 2*R + out (FFT downscale plans: S1, S2 of the cropped uW/2 + 1 columns, P->ncols)
    const double C = 3.0, W = P->W, H = P->H, uW = P->uW, uH = P->uH;
    const bool fused_u8 = fuse_u8(P);
    const double b_in = fused_u8 ? 1.0 : (double)P->esz;
    const double b_r = (double)P->esz, b_out = P->u8out ? 1.0 : b_r, b_c = (double)P->csz;
    const double in = C * W * H * b_in;
    const double S1 = C * P->ncols * H * b_c;
    const double S2 = C * P->ncols * uH * b_c;
    const double R = C * uW * uH * (P->cplx ? b_c : b_r);
    const double o = C * uW * uH * b_out;
    info->alg_bytes_per_frame = in + 2 * S1 + 2 * S2 + 2 * R + o;
    info->kernel_alg_bytes[0] = in + S1;
    info->kernel_alg_bytes[1] = S1 + S2;
    // a fused C2R+sharpen launch does the work of the reference's I2 and C dispatches: its algorithmic
    // bytes stay S2 + 2R + out although R never reaches HBM
    info->kernel_alg_bytes[2] = P->fused ? S2 + 2 * R + o : S2 + R;
    info->kernel_alg_bytes[3] = P->fused ? 0.0 : R + o;
    {
        // what the launches really have to move: polyphase plans write/read only the odd half of S2; a fused strip
        // re-reads one halo pair of spectrum rows
        const bool poly = (P->tuned || P->mixed) && P->U >= 2;
        const double S2w = poly ? S1 * (P->U - 1) : S2;               // odd rows (residues 1..U-1) only
        const double halo = P->fused ? (double)(P->pairs_per_strip + 1) / P->pairs_per_strip : 1.0;
        info->kernel_min_bytes[0] = in + S1;
        info->kernel_min_bytes[1] = S1 + S2w;
        info->kernel_min_bytes[2] = P->fused ? S2 * halo + o : S2 + R;
        info->kernel_min_bytes[3] = P->fused ? 0.0 : R + o;
    }
    if (P->dct) {
        // real coefficients instead of half spectra: S1 = [3][H][W], S2 = [3][uH][W] fp32 ("DCT upscale mode")
        const double D1 = C * W * H * 4.0, D2 = C * W * uH * 4.0;
        info->alg_bytes_per_frame = in + 2 * D1 + 2 * D2 + 2 * R + o;
        const double k[FFTUP_NUM_KERNELS] = {in + D1, D1 + D2, D2 + R, R + o};
        for (int i = 0; i < FFTUP_NUM_KERNELS; i++) info->kernel_alg_bytes[i] = info->kernel_min_bytes[i] = k[i];
    }
    info->device_bytes = P->device_bytes;
    info->abi_version = FFTUP_ABI_VERSION;
    info->u8_store = P->u8out ? 1 : 0;
    snprintf(info->device_name, sizeof info->device_name, "%s", device_label(P->prop));
    // (fftup_plan_create_size: the direction is a property of the axis, the row kernel crops when uW < W, the column kernel when uH < H)
    const bool crop_rows = P->exact ? P->uW < P->W : P->down, crop_cols = P->exact ? P->uH < P->H : P->down;
    const bool is_dct = P->family == fftup_plan::Family::dct, is_cplx = P->family == fftup_plan::Family::cplx;
    snprintf(info->kernel_names[0], 64, is_dct ? "dct_row" : crop_rows ? "row_r2c_crop" : is_cplx ? "row_c2c" : "row_r2c");
    snprintf(info->kernel_names[1], 64, is_dct ? (P->down ? "dct_col_crop_idct" : "dct_col_pad_idct") : crop_cols ? "col_fwd_crop_inv" : "col_fwd_pad_inv");
    snprintf(info->kernel_names[2], 64, is_dct ? "idct_row" : P->fused ? "row_c2r_sharpen" : (is_cplx ? "row_c2c_inv" : "row_c2r"));
    snprintf(info->kernel_names[3], 64, P->fused ? "-" : "sharpen");
    // S1 / S2 above hold P->ncols columns: W/2 + 1 with W/2 rounded DOWN (an odd W has (W + 1)/2 bins, none self-paired); odd plans
    // keep min(W, uW)/2 + 1.  The row kernels of an odd plan run (H + 1)/2 and (uH + 1)/2 workgroups per plane -- the rows are
    // rounded UP to pairs, the bytes are not: the tail workgroup moves one row.  Their names (kernels_odd.hpp):
    if (P->family == fftup_plan::Family::odd)
        for (int i = 0; i < 3; i++) strncat(info->kernel_names[i], "_odd", 63 - strlen(info->kernel_names[i]));
    if (P->family == fftup_plan::Family::view) {             // (kernels_view.hpp; the row R2C kernel is the odd-size plans')
        snprintf(info->kernel_names[0], 64, "row_r2c_odd");
        snprintf(info->kernel_names[1], 64, "col_view");
        snprintf(info->kernel_names[2], 64, "row_view_c2r");
    }
    // kernels with a Bluestein transform (kernels_bluestein.hpp)
    const bool kbz[3] = {P->bzW.L != 0, P->bzH.L != 0 || P->bzUH.L != 0, P->bzUW.L != 0};
    for (int i = 0; i < (P->family == fftup_plan::Family::view ? 2 : 3); i++)
        if (kbz[i]) strncat(info->kernel_names[i], "_bz", 63 - strlen(info->kernel_names[i]));
    return FFTUP_OK;
}

const char* fftup_strerror(int code)
{
    switch (code) {
    case FFTUP_OK: return "success";
    case FFTUP_E_INVALID_ARG: return "invalid argument";
    case FFTUP_E_UNSUPPORTED_SIZE: return "unsupported size (not 2,3,5,7-smooth)";
    case FFTUP_E_UNSUPPORTED_PRECISION: return "unsupported precision";
    case FFTUP_E_NO_DEVICE: return "no usable HIP device";
    case FFTUP_E_HIP: return "HIP runtime error";
    case FFTUP_E_OUT_OF_MEMORY: return "out of device memory";
    case FFTUP_E_NO_INPUT: return "no input uploaded / nothing executed";
    case FFTUP_E_INCOMPLETE: return "incomplete (image not found)";
    case FFTUP_E_WOULD_BLOCK: return "the call would wait for the calling thread itself";
    case FFTUP_E_OVERFLOW: return "an internal buffer bound was exceeded";
    default: return "unknown error";
    }
}

const char* fftup_last_error(void) { return g_last_error.c_str(); }
const char* fftup_version(void) { return "fftup 0.7.0 (gfx950, ABI 2)"; }

}  // extern "C"

// Plan-time tuner (FFTUP_FLAG_TUNE_PLAN / experiment jit_tune=1) for a run-time specialised plan: the chooser's alternatives for
// the fused C2R+sharpen kernel -- the one that takes two thirds of a frame -- are compiled and the PLAN is timed with
// each of them on this device, the way it will run (frames overlapping on the plan's streams when it has a ring of slots,
// else one after the other: a kernel that is faster alone but fills the compute units' registers makes overlapping
// frames slower), with the plan's own buffers (their contents do not matter: no data-dependent control flow).
// The fastest one is kept and remembered in <cache dir>/wisdom.txt, which later plans for the same row length, device
// and mode read instead of measuring again.  Different factorizations give the same pixels up to fp32 rounding (tests).
static void tune_fused(fftup_plan* P)
{
    const std::string arch = P->prop.gcnArchName;
    const fftup_jit::Choice base = P->jit->choice;
    const std::string key = fftup_jit::fused_key(base, wisdom_device_key(P));
    std::string known;
    if (fftup_jit::experiment("jit_fused") || fftup_jit::wisdom_lookup(key, known)) return;
    const std::vector<int> kinds = P->in_kind;
    const int executed = P->executed;
    for (auto& k : P->in_kind) if (!k) k = 1;                                  // (uninitialised planar input: fine for timing)
    const uint32_t frames = 4 * (uint32_t)std::max(1, std::min(P->nlanes, (int)P->ring));
    auto time_plan = [&]() -> double {
        double best = 1e30, ms = 0;
        for (int rep = 0; rep < 3; rep++) {
            if (execute_ring_impl(P, frames, 0, &ms, nullptr, 1) != FFTUP_OK) return 1e30;
            if (rep > 0) best = std::min(best, ms / frames);                    // (the first repetition warms up)
        }
        return best;
    };
    const double t_base = time_plan();
    if (t_base >= 1e30) {                                                       // the plan does not even run: nothing to learn, nothing to file
        P->in_kind = kinds;
        P->executed = executed;
        return;
    }
    double t_best = t_base;
    fftup_jit::Module* const original = P->jit;
    fftup_jit::Module* best = nullptr;
    // candidates: the chooser's alternatives -- and the structural default (pow2 / 16*16*R), when built-in wisdom made the
    // plan start from something else
    std::vector<fftup_jit::Choice> cands;
    {
        fftup_jit::Choice d;
        if (fftup_jit::choose(base.W, base.H, base.D, base.half, stage_radices(P->planUW), d, "", false, base.DD) &&
            fftup_jit::fused_value(d) != fftup_jit::fused_value(base)) {
            d.u8out = base.u8out;
            cands.push_back(d);
        }
    }
    for (const auto& cand : fftup_jit::fused_candidates(base.UW, base.D, 5, base.DD)) {
        if (base.fused_kind == 2 && cand.T == base.fused_t && cand.r == base.fr) continue;
        fftup_jit::Choice c = base;
        fftup_jit::set_fused_n(c, cand.T, cand.r);
        cands.push_back(c);
    }
    for (const fftup_jit::Choice& c : cands) {
        if (c.fused_lds > 160 * 1024) continue;
        std::string err;
        fftup_jit::Module* m = fftup_jit::load(c, arch, err);
        if (!m) continue;
        P->jit = m;
        set_strip_length(P);
        const double t = time_plan();
        P->jit = original;
        set_strip_length(P);
        if (getenv("FFTUP_JIT_VERBOSE"))
            fprintf(stderr, "fftup: tuning %s: %s %.1f us/frame (default %s %.1f)\n", key.c_str(), fftup_jit::fused_value(m->choice).c_str(), t * 1e3,
                    fftup_jit::fused_value(base).c_str(), t_base * 1e3);
        if (t < 0.97 * t_best) { delete best; best = m; t_best = t; }           // (3 %: do not chase noise)
        else delete m;
    }
    if (best) { delete original; P->jit = best; set_strip_length(P); }
    P->in_kind = kinds;
    P->executed = executed;
    fftup_jit::wisdom_store(key, fftup_jit::fused_value(P->jit->choice));
}
