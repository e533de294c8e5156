// fftup_plan.hip -- plan creation behind the C ABI (include/fftup.h): the request goes through the device-free planner
// (plan_rules.hpp: checks, then every decision), this unit opens the device, tries the plan-time compiler, fills the twiddle,
// chirp and phase tables, allocates the buffers and streams; destruction, fftup_plan_set_view, the plan-time tuner.  The kernels
// themselves are named in fftup_launch.hip only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "plan.hpp"
#include "mirror_tables.hpp"
#include "view_tables.hpp"

using namespace fftup;

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


// a table computed on the host (fp32 pairs, or double pairs behind the same pointer member): device memory owned by the plan,
// blocking copy
template <class T> static int upload_table(fftup_plan* P, float2** dptr, const std::vector<T>& h)
{
    int rc = dev_alloc(P, (void**)dptr, sizeof(T) * h.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpy(*dptr, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return FFTUP_OK;
}

// the n-th roots exp(+2 pi i k / n) in double (exact octant reduction is unnecessary there), rounded once to the plan's precision
template <class T> static std::vector<T> roots(uint32_t n)
{
    std::vector<T> h(n);
    for (uint32_t k = 0; k < n; k++) {
        const double a = 2.0 * M_PI * (double)k / (double)n;
        h[k].x = (decltype(h[k].x))std::cos(a); h[k].y = (decltype(h[k].y))std::sin(a);
    }
    return h;
}
static int make_twiddles(fftup_plan* P, float2** dptr, uint32_t n)
{
    return P->dbl ? upload_table(P, dptr, roots<double2>(n)) : upload_table(P, dptr, roots<float2>(n));
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


using fftup_viewtab::host_fft;                   // DFT with exp(+2 pi i nk / n) of a smooth length in double (view_tables.hpp)
// the tables of one Bluestein transform of n points through length L, in double, rounded once to fp32 (as make_twiddles).  The
// phase pi k^2 / n is reduced as (k^2 mod 2n) in 64-bit integers BEFORE the division: it reaches thousands of radians.
static int make_bluestein(fftup_plan* P, BzPlan* z, uint32_t n, uint32_t L)
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
    if (int rc = upload_table(P, &dc, hc)) return rc;
    if (int rc = upload_table(P, &db, hb)) return rc;
    if (int rc = make_twiddles(P, &dt, L)) return rc;
    z->L = (int32_t)L; z->plan = make_stage_plan(L); z->tw = dt; z->chirp = dc; z->bhat = db;
    return FFTUP_OK;
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
// Aim the plan at `v`: kmax per axis, the spectrum columns kept, the sharpen constant, the tables (blocking copies; the caller has
// made sure nothing of the plan is running).  An axis whose span did not change keeps its chirp tables: only `pre` holds the origin.
static int view_apply(fftup_plan* P, const fftup_view& v, bool first)
{
    struct Ax { fftup_plan::ViewAxis* a; uint32_t N, M; double o, sp, sp_old; };
    const Ax ax[2] = {{&P->vx, P->W, P->uW, v.origin_x, v.span_x, P->vw.span_x}, {&P->vy, P->H, P->uH, v.origin_y, v.span_y, P->vw.span_y}};
    for (const Ax& x : ax) {
        fftup_viewtab::AxisTables t;
        const bool chirp = first || x.sp != x.sp_old;
        if (P->mirror) fftup_viewtab::make_mirror_axis(x.N, x.M, x.o, x.sp, x.a->L, t, chirp);
        else fftup_viewtab::make_axis(x.N, x.M, x.o, x.sp, x.a->L, t, chirp);
        x.a->kmax = t.kmax;
        HIP_TRY(hipMemcpy(x.a->pre, t.pre.data(), sizeof(float) * t.pre.size(), hipMemcpyHostToDevice));
        if (chirp) {
            HIP_TRY(hipMemcpy(x.a->post, t.post.data(), sizeof(float) * t.post.size(), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(x.a->bhat, t.bhat.data(), sizeof(float) * t.bhat.size(), hipMemcpyHostToDevice));
        }
    }
    P->vw = v;
    P->ncols = P->mirror ? fftup_viewtab::mirror_ncols(P->W, P->vx.kmax) : P->vx.kmax + 1;
    P->NT = (P->ncols + P->TK - 1) / P->TK;
    P->cfg.upscale = view_factor(v, P->uW, P->uH);
    P->upsq = const_via_percent_f((double)(P->cfg.upscale * P->cfg.upscale), P->half);
    return FFTUP_OK;
}


// fftup_execute_device_views, on first use (like the device-I/O staging; the plan frees them): for the lanes [0, nl) a table set
// each with the sizes make_tables gives the plan's own, which k_view_tables fills per frame; per axis the L-th roots in double
// -- the table make_twiddles gives a -p 1 plan -- uploaded once; the kernel's LDS attribute
int view_frames_prepare(fftup_plan* P, int nl)
{
    if (P->vtabs.empty()) P->vtabs.resize(P->nlanes);
    const uint32_t len[4] = {P->W, P->H, P->uW, P->uH};
    const fftup_plan::ViewAxis* const axes[2] = {&P->vx, &P->vy};
    if (!P->vroots[0]) {
        if (int rc = kernels_allow_view_tables(P)) return rc;
        for (int i = 0; i < 2; i++) {
            float2* d = nullptr;
            if (int rc = upload_table(P, &d, roots<double2>(axes[i]->L))) return rc;
            P->vroots[i] = (double2*)d;
        }
    }
    for (int l = 0; l < nl; l++) {
        fftup_plan::ViewTabs& t = P->vtabs[l];
        for (int i = 0; i < 2 && !t.bhat[1]; i++) {
            if (int rc = dev_alloc(P, (void**)&t.pre[i], sizeof(float2) * (2 * (size_t)(P->mirror ? len[i] : len[i] / 2) + 1))) return rc;
            if (int rc = dev_alloc(P, (void**)&t.post[i], sizeof(float2) * len[2 + i])) return rc;
            if (int rc = dev_alloc(P, (void**)&t.bhat[i], sizeof(float2) * axes[i]->L)) return rc;
        }
    }
    return FFTUP_OK;
}


static void tune_fused(fftup_plan* P);
static bool jit_tune_enabled()
{
    const char* e = fftup_jit::experiment("jit_tune");
    return e && atoi(e) != 0;
}

// ---- plan creation, stage by stage
static int open_device(fftup_plan* P)
{
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(hipGetDeviceProperties(&P->prop, P->device));
    HIP_TRY(hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&P->ev0));
    HIP_TRY(hipEventCreate(&P->ev1));
    return FFTUP_OK;
}

// the plan-time compiler's attempt (plan_jit_factor: does the plan ask for it?): kernels specialised for this size on this
// device, or nullptr -- the size-generic kernels run the plan
static fftup_jit::Module* specialise(const fftup_plan* P, const DeviceFacts& dev)
{
    int DD = 1;
    const int D = plan_jit_factor(*P, &DD);
    fftup_jit::Choice ch;
    if (!D || !fftup_jit::choose((int)P->W, (int)P->H, D, P->half, stage_radices(P->planUW), ch, wisdom_device_key(*P, dev), true, DD)) return nullptr;
    ch.u8out = (P->cfg.flags & FFTUP_FLAG_FUSE_U8_STORE) != 0;         // (such a plan is always fused)
    std::string jerr;
    fftup_jit::Module* m = fftup_jit::load(ch, dev.arch, jerr);
    if (!m && getenv("FFTUP_JIT_VERBOSE")) fprintf(stderr, "fftup: run-time specialisation failed, size-generic kernels in use: %s\n", jerr.c_str());
    return m;
}

// every table the plan's kernels read: roots, four-step roots, Bluestein, phase, chirp-z and DCT tables
static int make_tables(fftup_plan* P)
{
    const uint32_t len[4] = {P->W, P->H, P->uW, P->uH};
    float2** const tw[4] = {&P->twW, &P->twH, &P->twUW, &P->twUH};
    for (int i = 0; i < 4; i++)
        if (int rc = make_twiddles(P, tw[i], len[i])) return rc;
    const std::pair<const fftup_plan::Four*, fftup_plan::FourTables*> fours[4] = {{&P->fourF, &P->fourFtw}, {&P->fourI, &P->fourItw}, {&P->colF, &P->colFtw}, {&P->colI, &P->colItw}};
    for (auto& f : fours) {
        if (!f.first->on) continue;
        if (int rc = make_twiddles(P, &f.second->tw1, (uint32_t)f.first->n1)) return rc;
        if (int rc = make_twiddles(P, &f.second->tw2, (uint32_t)f.first->n2)) return rc;
    }
    BzPlan* const bz[4] = {&P->bzW, &P->bzH, &P->bzUW, &P->bzUH};
    for (int i = 0; i < 4; i++)
        if (P->bzL[i])
            if (int rc = make_bluestein(P, bz[i], len[i], P->bzL[i])) return rc;
    if (P->exact && P->align == FFTUP_ALIGN_CENTRE) {
        if (int rc = make_phases(P, &P->phW, P->W, P->uW)) return rc;
        if (int rc = make_phases(P, &P->phH, P->H, P->uH)) return rc;
    }
    if (P->view) {
        // tables of the worst case: 2 (N/2) + 1 bins in (mirror plans: 2 N + 1, the doubled period's), M points out, L points of the
        // convolution
        fftup_plan::ViewAxis* const axes[2] = {&P->vx, &P->vy};
        for (int i = 0; i < 2; i++) {
            fftup_plan::ViewAxis& a = *axes[i];
            a.L = P->viewL[i]; a.planL = make_stage_plan(a.L);
            if (int rc = make_twiddles(P, &a.tw, a.L)) return rc;
            if (int rc = dev_alloc(P, (void**)&a.pre, sizeof(float2) * (2 * (size_t)(P->mirror ? len[i] : len[i] / 2) + 1))) return rc;
            if (int rc = dev_alloc(P, (void**)&a.post, sizeof(float2) * len[2 + i])) return rc;
            if (int rc = dev_alloc(P, (void**)&a.bhat, sizeof(float2) * a.L)) return rc;
        }
    }
    if (P->mirror) {                                   // exp(i pi k / 2n) of the two input lengths (kernels_mirror.hpp)
        if (int rc = make_rotations(P, &P->rotW, P->W)) return rc;
        if (int rc = make_rotations(P, &P->rotH, P->H)) return rc;
    }
    if (P->dct) {
        float2** const rot[4] = {&P->rotW, &P->rotH, &P->rotUW, &P->rotUH};
        for (int i = 0; i < 4; i++)
            if (int rc = make_rotations(P, rot[i], len[i])) return rc;
    }
    return FFTUP_OK;
}

// the spectra of one lane.  Tuned plans (k_col_t): S2 holds the odd rows only and sits right behind S1 in ONE allocation (the
// fused kernel addresses both with 32-bit offsets from one base)
static int alloc_spectra(fftup_plan* P, float2** s1, float2** s2)
{
    const size_t s1_elems = (size_t)3 * P->NT * P->H * P->TK;
    if ((P->tuned || P->mixed) && P->U >= 2) {
        int r = dev_alloc(P, (void**)s1, P->csz * (size_t)P->U * s1_elems);       // S1 + the U-1 residue buffers
        *s2 = r ? nullptr : *s1 + s1_elems;
        return r;
    }
    int r = dev_alloc(P, (void**)s1, P->csz * s1_elems);
    return r ? r : dev_alloc(P, (void**)s2, P->csz * 3 * (size_t)P->NT * P->uH * P->TK);
}

// the ring's input and output slots, lane 0's spectra, the pre-sharpen image, the 8-bit staging
static int make_buffers(fftup_plan* P)
{
    const size_t esz = P->esz, out_pixels = (size_t)3 * P->uW * P->uH;
    P->in_plane_stride = (size_t)(P->W + 2) * P->H;              // VkResample.cpp:1644
    P->in_planar.assign(P->ring, nullptr);
    P->in_u8.assign(P->ring, nullptr);
    P->in_kind.assign(P->ring, 0);
    P->out.assign(P->ring, nullptr);
    for (uint32_t s = 0; s < P->ring; s++) {
        if (int rc = dev_alloc(P, &P->in_planar[s], 3 * P->in_plane_stride * esz)) return rc;
        if (int rc = dev_alloc(P, (void**)&P->in_u8[s], (size_t)3 * P->W * P->H)) return rc;
        if (int rc = dev_alloc(P, &P->out[s], out_pixels * (P->u8out ? 1 : esz) + 8)) return rc;          // (+ 8: readers of whole words)
    }
    P->r_bytes = out_pixels * (P->cplx ? (P->half ? 4 : P->csz) : esz);  // non-R2C path: complex pre-sharpen image (binary16 pairs for -p 2)
    if (!P->u8out)
        if (int rc = dev_alloc(P, (void**)&P->out_u8, out_pixels + 8)) return rc;   // staging of the conversion launch (+ 8: k_png_filter reads whole words)
    return FFTUP_OK;
}

// the streams consecutive frames alternate on: lane 0 runs on the plan's own stream, every other lane on its own; each lane has
// its spectra and its completion event.  The pre-sharpen image R (the reference's tempBuffer): every frame of an unfused plan
// goes through it; a fused plan only needs one for the fftup_download_presharpen tap, which allocates it on first use
static int make_lanes(fftup_plan* P)
{
    P->nlanes = lane_count();
    P->lanes.resize(P->nlanes);
    const size_t t4_bytes = P->csz * 3 * std::max(std::max(P->fourF.on ? (size_t)P->W * P->H : 0, P->fourI.on ? (size_t)P->uW * P->uH : 0),
                                                  P->colI.on ? (size_t)P->ncols * P->uH : 0);
    for (int l = 0; l < P->nlanes; l++) {
        fftup_plan::Lane& lane = P->lanes[l];
        if (l == 0) lane.stream = P->stream;
        else HIP_TRY(hipStreamCreateWithFlags(&lane.stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&lane.done, hipEventDisableTiming));
        if (int rc = alloc_spectra(P, &lane.S1, &lane.S2)) return rc;
        if (!P->fused)
            if (int rc = dev_alloc(P, &lane.R, P->r_bytes)) return rc;
        if (t4_bytes)
            if (int rc = dev_alloc(P, &lane.T4, t4_bytes)) return rc;
    }
    return FFTUP_OK;
}

// the plan under construction: destroyed on every early return
struct PlanDestroyer { void operator()(fftup_plan* P) const { fftup_plan_destroy(P); } };

static int plan_create(fftup_plan** out, const PlanRequest& rq)
{
    if (!out || !rq.cfg) return fail(FFTUP_E_INVALID_ARG, "null argument");
    *out = nullptr;
    PlanGeometry G;
    if (int rc = plan_check(rq, G)) return rc;               // (before any device access)
    const int ndev = fftup_device_count();
    if (ndev <= 0) return fail(FFTUP_E_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (G.cfg.device < 0 || G.cfg.device >= ndev) return fail(FFTUP_E_NO_DEVICE, "device id out of range");

    std::unique_ptr<fftup_plan, PlanDestroyer> owner(new fftup_plan());
    fftup_plan* const P = owner.get();
    static_cast<PlanGeometry&>(*P) = G;
    P->device = G.cfg.device;
    if (int rc = open_device(P)) return rc;
    const DeviceFacts dev = device_facts(P->prop);
    if (int rc = plan_geometry_columns(*P, dev)) return rc;
    P->jit = specialise(P, dev);
    if (int rc = plan_geometry_finish(*P, dev, P->jit ? &P->jit->choice : nullptr)) return rc;
    if (int rc = make_tables(P)) return rc;
    if (int rc = make_buffers(P)) return rc;
    if (int rc = make_lanes(P)) return rc;
    if (rq.view)
        if (int rc = view_apply(P, *rq.view, true)) return rc;       // (after the allocations above: they are the worst case's)
    if (int rc = kernels_set_attributes(P)) return rc;               // dynamic LDS above 64 KB for the kernels THIS plan launches (fftup_launch.hip)
    if (P->mixed == 3 && ((P->cfg.flags & FFTUP_FLAG_TUNE_PLAN) || jit_tune_enabled())) tune_fused(P);
    png_geometry(P);                       // (fixed per plan: fftup_png_bound may be asked by several threads at once)
    *out = owner.release();
    return FFTUP_OK;
}

// ------------------------------------------------------------------------------------------------
extern "C" {

int fftup_plan_create(fftup_plan** out, const fftup_config* cfg) { return plan_create(out, {cfg, nullptr, 0, nullptr}); }

int fftup_plan_create_size(fftup_plan** out, const fftup_config* cfg, uint32_t out_width, uint32_t out_height, uint32_t align)
{
    const uint32_t size[2] = {out_width, out_height};
    return plan_create(out, {cfg, size, align, nullptr});
}

int fftup_plan_create_view(fftup_plan** out, const fftup_config* cfg, uint32_t out_width, uint32_t out_height, const fftup_view* view)
{
    if (out) *out = nullptr;
    if (!out || !cfg || !view) return fail(FFTUP_E_INVALID_ARG, "null argument");
    const uint32_t size[2] = {out_width, out_height};
    return plan_create(out, {cfg, size, FFTUP_ALIGN_CORNER, view});
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


int fftup_jit_check(uint32_t width, uint32_t height, float upscale, uint32_t precision, const char* arch, char* desc, size_t desclen)
{
    if (desc && desclen) desc[0] = 0;
    if (precision != 0 && precision != 2) return fail(FFTUP_E_UNSUPPORTED_PRECISION, "run-time specialised plans exist for -p 0 and -p 2");
    if (width < 2 || height < 2 || (width & 1) || (height & 1) || width > 65536 || height > 65536 || !is_smooth(width) || !is_smooth(height))
        return fail(FFTUP_E_UNSUPPORTED_SIZE, "sizes must be even and factor into 2,3,5,7");
    fftup_jit::Choice ch;
    if (!(upscale >= 1.0f && upscale <= 8.0f)) return fail(FFTUP_E_INVALID_ARG, "upscale out of range");
    const uint32_t uW = scaled_length(upscale, width), uH = scaled_length(upscale, height);
    int DD = 1, zly = 0, zry = 0;
    column_guard(upscale, uH, &zly, &zry);
    const int D = (uW & 1) || (uH & 1) || !is_smooth(uW) || !is_smooth(uH) || uW > 8192 ? 0 : jit_factor(upscale, width, height, uW, uH, zly, zry, &DD);
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
    for (size_t l = 0; l < P->lanes.size(); l++) {           // (lane 0's stream is the plan's own: destroyed below)
        if (l && P->lanes[l].stream) { (void)hipStreamSynchronize(P->lanes[l].stream); (void)hipStreamDestroy(P->lanes[l].stream); }
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
    for (void* p : P->allocs) (void)hipFree(p);
    delete P->jit;
    if (P->ev0) (void)hipEventDestroy(P->ev0);
    if (P->ev1) (void)hipEventDestroy(P->ev1);
    if (P->stream) (void)hipStreamDestroy(P->stream);
    delete P;
}


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
    const DeviceFacts dev = device_facts(P->prop);
    const std::string& arch = dev.arch;
    const fftup_jit::Choice base = P->jit->choice;
    const std::string key = fftup_jit::fused_key(base, wisdom_device_key(*P, dev));
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
    auto use = [&](fftup_jit::Module* m) { P->jit = m; P->pairs_per_strip = strip_length(*P, dev, m->choice.fused_t); };   // (launches take P->jit as it is)
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
        use(m);
        const double t = time_plan();
        use(original);
        if (getenv("FFTUP_JIT_VERBOSE"))
            fprintf(stderr, "fftup: tuning %s: %s %.1f us/frame (default %s %.1f)\n", key.c_str(), fftup_jit::fused_value(m->choice).c_str(), t * 1e3,
                    fftup_jit::fused_value(base).c_str(), t_base * 1e3);
        if (t < 0.97 * t_best) { delete best; best = m; t_best = t; }           // (3 %: do not chase noise)
        else delete m;
    }
    if (best) { delete original; use(best); }
    P->in_kind = kinds;
    P->executed = executed;
    fftup_jit::wisdom_store(key, fftup_jit::fused_value(P->jit->choice));
}
