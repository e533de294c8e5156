// plan_rules.hpp / plan_rules.cpp -- the planner without a device: what a request (configuration, optional output size, optional
// view) is checked against and every decision a plan holds about its kernels -- sizes, zero-padding ranges, the R2C rule,
// factorizations (launchResample's plan semantics, VkResample.cpp:1409-1617), column tile width, LDS bytes, threads, four-step
// splits, in-place variants, strip length, the kernel family.  Arithmetic on the request and three facts about the device; no HIP
// runtime call.  fftup_plan.hip runs it between opening the device and filling the tables; tests/plan_rules_driver.cpp runs it
// without a device.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fftup.h"
#include "fft_engine.hpp"
#include "jit_choose.hpp"

using fftup::StagePlan;

static constexpr int TUNED_TK = 4;     // column tile width of the size-specialised kernels

// ---- errors: code + thread-local detail (fftup_last_error; fftup_info.hip)
int fail(int code, const std::string& msg);

// facts about the kernels the planner needs (defined next to the kernels, fftup_launch.hip)
int kernels_generic_max_threads(bool dbl);                        // threads per workgroup of the size-generic kernels
int kernels_aot_mixed_plan(uint32_t W, uint32_t H);               // 1: 1920x1080, 2: 1280x720 (ahead-of-time mixed-radix plans), 0: none
size_t kernels_tuned_col_lds(uint32_t H);                         // LDS bytes of the power-of-two column kernel

// what the planner knows about the device (hipDeviceProp_t: sharedMemPerBlock, multiProcessorCount, gcnArchName)
struct DeviceFacts { size_t lds_bytes = 0; int compute_units = 0; std::string arch; };

// fftup_plan_create (size == nullptr: the output size follows from cfg->upscale), fftup_plan_create_size (size = {uW, uH},
// cfg->upscale ignored) and fftup_plan_create_view (size and view)
struct PlanRequest { const fftup_config* cfg = nullptr; const uint32_t* size = nullptr; uint32_t align = 0; const fftup_view* view = nullptr; };

// the decisions of a plan: plain data, filled by plan_check and plan_geometry; fftup_plan (plan.hpp) adds what lives on the device
struct PlanGeometry {
    fftup_config cfg{};
    uint32_t W = 0, H = 0, uW = 0, uH = 0;
    uint32_t ring = 1;
    bool half = false;                // -p 2: binary16 storage
    bool dbl = false;                 // -p 1: double storage and arithmetic (size-generic kernels, double2 spectra)
    size_t esz = 4, csz = 8;          // bytes per real / complex element in HBM

    int TK = 8, NT = 0;
    int zlx = 0, zrx = 0, zly = 0, zry = 0;
    StagePlan planW{}, planH{}, planUW{}, planUH{};
    int thrW = 0, thrCol = 0, thrUW = 0;
    size_t ldsRowF = 0, ldsCol = 0, ldsRowI = 0;
    float upsq = 0, coef = 0;
    // Which set of kernels runs the frame: decided ONCE, by plan_geometry, from the fields below (which stay: they also describe
    // properties that cut across the families -- half, bz, exact, poly, fused, u8out, inplace*, down together with dct).  What
    // launches, attributes and descriptions branch on.  generic: size-generic R2C kernels on fp32 / fp16 data; tuned: ahead-of-time
    // power-of-two kernels; mixed_aot / mixed_jit: mixed-radix kernels compiled ahead of time / at plan time (`mixed` 1, 2 / 3);
    // cplx: non-R2C path (either precision); f64: -p 1 R2C; dct (up or down); down: FFT downscale; odd: odd and exact sizes; view
    enum class Family { generic, tuned, mixed_aot, mixed_jit, cplx, f64, dct, down, odd, view };
    Family family = Family::generic;
    bool tuned = false;
    bool fused = false;               // sharpen fused into the C2R kernel (tuned plans)
    bool u8out = false;               // FFTUP_FLAG_FUSE_U8_STORE in effect: the fused kernel stores 8-bit RGB, `out` slots hold [uH][uW][3] bytes
    int mixed = 0;                    // compile-time mixed-radix plans: 1 = 1920x1080 -> 3840x2160, 2 = 1280x720 -> 2560x1440,
                                      // 3 = specialised at plan time for this size (jit.hpp), kernels in fftup_plan::jit
    int U = 2;                        // integer upscale factor of a polyphase plan (tuned / mixed): S1 + U-1 residue buffers
    bool cplx = false;                // non-R2C path (VR:1424 false): full complex transforms, uW beyond the R2C limit
    bool dct = false;                 // FFTUP_FLAG_DCT: DCT-II -> zero-pad -> DCT-III (kernels_dct.hpp); S1 / S2 hold real [3][H][W] / [3][uH][W]
    bool down = false;                // FFTUP_FLAG_DOWNSCALE: uW < W, uH < H; without dct the spectrum is cropped (kernels_downscale.hpp): ncols = uW/2 + 1
    bool poly = false;                         // size-generic u = 2 plan: polyphase column kernel (k_col_poly), the C2R kernel reads the even rows from S1
    bool inplaceC = false;                     // -p 1 R2C plans: the column kernel's two transforms in one LDS buffer (k_col<TK, double2, true>)
    bool inplaceF = false, inplaceI = false;   // ... whose forward / inverse rows are too long for two LDS buffers: fft_lds_inplace
    // ... and rows too long for ONE buffer: four steps through HBM (k_row4_a / k_row4_b), row length = n1 * n2 (their twiddle
    // tables: fftup_plan::FourTables)
    struct Four { bool on = false; int n1 = 0, n2 = 0, tka = 1, tkb = 1;    // N = n1 * n2; sequences per workgroup of pass A / pass B
                  StagePlan p1{}, p2{}; size_t ldsA = 0, ldsB = 0; int thrA = 64, thrB = 64; };
    Four fourF, fourI;
    Four colF, colI;                  // columns longer than the LDS (TK = 1): the same two kernels on dense columns
    // FFTUP_FLAG_ANY_SIZE: per transform (W, H, uW, uH), L != 0 = the length has a prime factor above 7 and runs as a Bluestein
    // transform of length L (kernels_bluestein.hpp; the tables: fftup_plan::bzW ..); `bz`: the plan has at least one such transform
    // (size-generic R2C kernels, fp32 arithmetic)
    uint32_t bzL[4] = {0, 0, 0, 0};
    bool bz = false;
    // FFTUP_FLAG_ODD_SIZE with an odd W, H, uW or uH: exact trigonometric resampling on both axes (kernels_odd.hpp), up, down or
    // -u 1; ncols = min(W, uW)/2 + 1 (floor); (rows + 1)/2 workgroups per plane in the row kernels
    bool odd = false;
    // fftup_plan_create_size: the output size is given per axis (always `odd`'s kernels, each axis up, down or equal on its own);
    // align = FFTUP_ALIGN_CENTRE: phase tables of the axes whose lengths differ (kernels_odd.hpp)
    bool exact = false;
    uint32_t align = 0;
    // fftup_plan_create_view: the frame's trigonometric interpolant at origin + m span / M per axis (kernels_view.hpp).  Buffers and
    // the convolution lengths are sized for the worst case of W, H, uW, uH (kmax = N/2), so fftup_plan_set_view re-aims the plan in
    // place; ncols = kmax_x + 1 and NT follow the CURRENT view (fftup_plan::vx, vy).  viewL: the smooth convolution length per axis
    bool view = false;
    uint32_t viewL[2] = {0, 0};
    // ... with FFTUP_FLAG_MIRROR: the view of the frame's half-sample even reflection (kernels_mirror.hpp).  Still Family::view -- the
    // same passes, buffers and fftup_plan_set_view; the selectors of fftup_launch.hip hand out the mirror kernels.  viewL are the
    // convolution lengths of the doubled periods (>= 2N + M), ncols = kmax_x + 1 below W/2, else W/2 + 1 (mirror_tables.hpp)
    bool mirror = false;
    int ncols = 0;                    // spectrum columns kept: W/2 + 1, or W on the non-R2C path
    int pairs_per_strip = 6;
};

// Everything a request is checked against, before any device access: the arguments, the output sizes, the modes and what they
// exclude, the effective factor of exact-size and view plans, whether rows and columns of these lengths can run at all (gfx950:
// 160 KB of LDS per workgroup).  Fills the request's part of G: cfg, sizes, storage, modes, ncols.
int plan_check(const PlanRequest& rq, PlanGeometry& G);
// The decisions, in two steps around the plan-time compiler's attempt (`mixed == 3` depends on whether its kernels loaded):
// plan_geometry_columns -- padding ranges, radix lists, tuned / ahead-of-time mixed kernels, column tile width and column LDS;
// plan_jit_factor -- does the plan ask for kernels specialised at plan time?  2 DD x factor (0: no), see jit_factor;
// plan_geometry_finish -- with the Choice whose kernels loaded (nullptr: none): family, fusion, strip length, rows, threads
int plan_geometry_columns(PlanGeometry& G, const DeviceFacts& dev);
int plan_jit_factor(const PlanGeometry& G, int* DD);
int plan_geometry_finish(PlanGeometry& G, const DeviceFacts& dev, const fftup_jit::Choice* jit);

// row pairs per strip of the fused C2R+sharpen kernel when it runs with `fused_threads` threads (G.pairs_per_strip: plan_geometry_finish)
int strip_length(const PlanGeometry& G, const DeviceFacts& dev, int fused_threads);
// what the tuner's findings are filed under: the device and whether consecutive frames overlap or run one after the other
std::string wisdom_device_key(const PlanGeometry& G, const DeviceFacts& dev);
int lane_count();                                                 // FFTUP_STREAMS: HIP streams ("lanes") the frames of a plan alternate on

// ---- arithmetic shared with plan creation (fftup_plan.hip)
bool is_smooth(uint32_t n);                                       // factors into 2, 3, 5, 7
StagePlan make_stage_plan(uint32_t n);
std::vector<int> stage_radices(const StagePlan& p);
uint32_t scaled_length(float upscale, uint32_t n);                // VkResample.cpp:1417-1418
void column_guard(float upscale, uint32_t uH, int* zly, int* zry);   // the zero-padding range of the column pass (VkResample.cpp:1494-1495)
int jit_factor(float upscale, uint32_t W, uint32_t H, uint32_t uW, uint32_t uH, int zly, int zry, int* DD);
int check_view(const char* who, const fftup_view* v, uint32_t uW, uint32_t uH);
float view_factor(const fftup_view& v, uint32_t uW, uint32_t uH);

// ---- fftup_align_create: every rule and decision of an aligner (include/fftup.h, "shift estimates"), before any device access.
// Kx, Ky: the bins in band per axis -- signed k in [-n/2, n/2) with |k| <= band_k, index i = k + band_k; K = Kx Ky
struct AlignGeometry {
    uint32_t W = 0, H = 0, precision = 0, nx = 0, ny = 0, d = 1, crop_x = 0, crop_y = 0, kappa = 32, band_kx = 0, band_ky = 0;
    uint32_t Kx = 0, Ky = 0, max_batch = 16;
    float band = 0.5f;
};
int align_geometry(const fftup_align_config& c, AlignGeometry& G);

// ---- fftup_rotate_create: every rule and decision of a rotator (include/fftup.h, "rotation by three shears"), before any device
// access.  TK: adjacent columns per workgroup of the column pass; lds_x / lds_y: dynamic LDS of the row / column kernels in bytes
struct RotateGeometry {
    uint32_t W = 0, H = 0, precision = 0, max_batch = 4, TK = 4;
    size_t lds_x = 0, lds_y = 0;
};
int rotate_geometry(const fftup_rotate_config& c, RotateGeometry& G);
float const_via_percent_f(double v, bool half);

// ---- fftup_roll_create: every rule and decision of a roll estimator (include/fftup.h, "roll estimates"), before any device access.
// n = min(nx, ny); ntheta: angular samples over [0, pi); rho_min .. rho_max: the radii sampled, in bins of the transform padded to
// 2 nx x 2 ny; mb: the angular frequencies 1 <= |m| <= mb that are correlated, K = 2 mb of them.  cx, cy: the largest |k_x| and k_y a
// sample's lower-left bin can have (rho_max nx / n, rho_max ny / n): columns -cx - 1 .. cx + 1 and rows 0 .. cy + 1 are computed
struct RollGeometry {
    uint32_t W = 0, H = 0, precision = 0, nx = 0, ny = 0, d = 1, crop_x = 0, crop_y = 0, kappa = 32, max_batch = 16;
    uint32_t n = 0, ntheta = 0, rho_min = 0, rho_max = 0, mb = 0, K = 0, cx = 0, cy = 0;
    float band = 0.5f;
};
int roll_geometry(const fftup_roll_config& c, RollGeometry& G);
