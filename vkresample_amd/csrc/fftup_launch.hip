// fftup_launch.hip -- the frame's kernel launches: the ONLY translation unit that instantiates the frame kernels (kernels_*.hpp).
// One frame = row R2C -> column FFT / zero-pad / iFFT -> row C2R + sharpen (fused) on the stream of the lane its caller names; the
// reference's 20 dispatches per frame (performVulkanUpscale, VkResample.cpp:1249-1279).
// Layout: (1) the kernel selectors -- per pass and plan family ONE function from the plan's fields (and the input kind) to the
// kernel instantiation with its block size and dynamic LDS bytes; (2) kernels_set_attributes, which asks the selectors for
// every kernel the plan can launch and allows it those bytes; (3) the frame functions per family, functions of (const plan,
// Frame, Pass), which ask the same selectors, compute grid and parameters per launch and launch; (4) launch_frame, which
// resolves its caller's FrameRun into the Frame, switches on P->family, and alone records what the frame left in the plan
// (last_lane, R_valid).  A kernel instantiation is spelled in its selector and nowhere else.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "plan.hpp"
#include "kernels_generic.hpp"
#include "kernels_pow2.hpp"
#include "kernels_mixed.hpp"
#include "kernels_dswap.hpp"
#include "kernels_dct.hpp"
#include "kernels_downscale.hpp"
#include "kernels_bluestein.hpp"
#include "kernels_odd.hpp"
#include "kernels_view.hpp"
#include "kernels_mirror.hpp"
#include "kernels_view_tables.hpp"
#include "kernels_path.hpp"
#include "kernels_device_io.hpp"
#include "mirror_tables.hpp"

using namespace fftup;
using Family = fftup_plan::Family;

// ---- facts about the kernels the planner needs
int kernels_generic_max_threads(bool dbl) { return dbl ? GenericMaxThreads<double2>::value : GenericMaxThreads<float2>::value; }
int kernels_aot_mixed_plan(uint32_t W, uint32_t H)
{
    if (W == MixedCfg1080::W && H == MixedCfg1080::H) return 1;
    if (W == MixedCfg720::W && H == MixedCfg720::H) return 2;
    return 0;
}
size_t kernels_tuned_col_lds(uint32_t H) { return sizeof(float2) * (size_t)lswz_size((int)H * TUNED_TK); }   // both transforms of the column kernel have length H

// One frame as the frame functions see it, a FrameRun resolved once by launch_frame: the lane's stream and buffers, where the first kernel
// reads (a ring slot or the caller's DeviceInput; kind 1 planes, 2 8-bit RGB, 0 nothing uploaded) and where the last one writes
// -- and what follows the frame's view: the spectrum columns kept (ncols, NT), the sharpen constant upsq, and for view plans kmax and
// the chirp tables per axis.  Filled from the plan; a FrameRun with a view of its own replaces them (frame_view below)
struct ViewTables { int kmax; const float2 *pre, *post, *bhat; };
struct Frame { hipStream_t st; float2 *S1, *S2; void *R, *T4; const void* in; long in_row, in_plane; int kind; void* out;
               int ncols, NT; float upsq; ViewTables vx, vy; };
static Frame resolve(const fftup_plan* P, const FrameRun& r)
{
    const fftup_plan::Lane& l = P->lanes[r.lane];
    Frame f{l.stream, l.S1, l.S2, l.R, l.T4, P->in_planar[r.in_slot], (long)P->W, (long)P->in_plane_stride, P->in_kind[r.in_slot], r.out,
            P->ncols, P->NT, P->upsq, {P->vx.kmax, P->vx.pre, P->vx.post, P->vx.bhat}, {P->vy.kmax, P->vy.pre, P->vy.post, P->vy.bhat}};
    if (r.in) { f.in = r.in->in; f.in_row = r.in->in_row; f.in_plane = r.in->kind == 2 ? 0 : r.in->in_plane; f.kind = r.in->kind; }
    else if (f.kind == 2) { f.in = P->in_u8[r.in_slot]; f.in_row = 3l * P->W; f.in_plane = 0; }
    return f;
}
template <class Q> static void set_in(const Frame& f, Q& q) { q.in = f.in; q.in_row_stride = f.in_row; q.in_plane_stride = f.in_plane; }   // a forward row kernel's input
static bool runs(Pass pass, Pass k) { return pass == Pass::all || pass == k; }

// ------------------------------------------------------------------------------------------------
// A kernel as a selector hands it out: what may be resolved ahead of a launch (grids and parameters are the launch's business:
// fftup_plan_set_view changes NT / ncols / kmax on a live plan, lane and images change per frame)
template <class... A> struct Kern { void (*fn)(A...); unsigned block; size_t lds; };
template <class... A> static Kern<A...> kern(void (*fn)(A...), int block, size_t lds) { return {fn, (unsigned)block, lds}; }
template <class T> struct type_c { using type = T; };
// (a failed launch is found by frame_status at the end of the frame, as with the triple-chevron form of the same runtime call)
template <class... A> static void launch(const Kern<A...>& k, dim3 grid, hipStream_t st, const typename type_c<A>::type&... a)
{
    void* args[] = {const_cast<void*>((const void*)&a)...};
    (void)hipLaunchKernel((const void*)k.fn, grid, dim3(k.block), args, k.lds, st);
}
// the two passes of a four-step transform (k_row4_a / k_row4_b; they pick their tile widths independently)
template <typename C> struct FourKerns { Kern<Row4Params<C>> a, b; };

// a run-time field of the plan as a compile-time constant: f(std::integral_constant) -- the tile width (MAX, MAX/2 .. 1; anything
// else runs as 1), a flag, the input mode of a forward row kernel (8-bit RGB or planes, binary16 or fp32 storage), the
// ahead-of-time mixed-radix configuration
template <int MAX = 8, class F> static auto with_tile(int tk, F&& f)
{
    if constexpr (MAX > 1) {
        if (tk == MAX) return f(std::integral_constant<int, MAX>{});
        return with_tile<MAX / 2>(tk, f);
    }
    else return f(std::integral_constant<int, 1>{});
}
template <class F> static auto with_flag(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> static auto with_mode(bool half, int kind, F&& f)
{
    if (kind == 2) return half ? f(std::integral_constant<int, IN_U8_F16>{}) : f(std::integral_constant<int, IN_U8_F32>{});
    return half ? f(std::integral_constant<int, IN_F16>{}) : f(std::integral_constant<int, IN_F32>{});
}
template <class F> static auto with_mixed_cfg(const fftup_plan* P, F&& f) { return P->mixed == 1 ? f(type_c<MixedCfg1080>{}) : f(type_c<MixedCfg720>{}); }

// ---- the selectors.  `kind`: the input kind of the frame (1 planes, 2 8-bit RGB).  A selector returns the kernel -- except
// where the kernels of one pass differ in their trailing arguments (the Bluestein forms take their BzPlans after the parameter
// struct), so that no single Kern type holds them: generic_c2r_kernel and columns_kernel call
// f(kernel, the arguments after the parameter struct...) instead, and launch and attribute setter pass their action as f.
// size-generic R2C plans, fp32 / fp16 (kernels_generic.hpp; a Bluestein transform on the axis: kernels_bluestein.hpp, and for
// the forward rows the resampling row kernel -- resampling_rows below)
static Kern<RowR2CParams> generic_row_kernel(const fftup_plan* P, int kind)
{
    return with_mode(P->half, kind, [&](auto m) { return kern(k_row_r2c<m()>, P->thrW, P->ldsRowF); });
}
// (also the inverse rows of an FFT downscale plan)
template <class F> static auto generic_c2r_kernel(const fftup_plan* P, F&& f)
{
    return with_flag(P->half, [&](auto h) {
        if (P->bzUW.L) return f(kern(k_row_c2r_bz<h()>, P->thrUW, P->ldsRowI), P->bzUW);
        return f(kern(k_row_c2r<h()>, P->thrUW, P->ldsRowI));
    });
}
// columns in LDS of the size-generic plans on C (R2C and non-R2C): polyphase, in place in one buffer (-p 1) or two buffers
// (plan_create sets neither poly nor inplaceC on the non-R2C path: those plans get k_col<TK, C>)
template <typename C> static Kern<ColParamsT<C>> col_kernel(const fftup_plan* P)
{
    return with_tile(P->TK, [&](auto tk) {
        if (P->poly) return kern(k_col_poly<tk(), C>, P->thrCol, P->ldsCol);
        if constexpr (sizeof(scalar_t<C>) == 8) {
            if (P->inplaceC) return kern(k_col<tk(), C, true>, P->thrCol, P->ldsCol);
        }
        return kern(k_col<tk(), C, false>, P->thrCol, P->ldsCol);
    });
}
// ... or, fp32 plans with a Bluestein column transform, k_col_bz
template <typename C, class F> static auto columns_kernel(const fftup_plan* P, F&& f)
{
    if constexpr (sizeof(scalar_t<C>) == 4) {
        if (P->bzH.L || P->bzUH.L) return with_tile(P->TK, [&](auto tk) { return f(kern(k_col_bz<tk()>, P->thrCol, P->ldsCol), P->bzH, P->bzUH); });
    }
    return f(col_kernel<C>(P));
}
// -p 1: the size-generic kernels on double2, rows in one LDS buffer where their stages run in place
static Kern<RowR2CParamsT<double2>> f64_row_kernel(const fftup_plan* P)
{
    return with_flag(P->inplaceF, [&](auto ip) { return kern(k_row_r2c<IN_F64, double2, ip()>, P->thrW, P->ldsRowF); });
}
static Kern<RowC2RParamsT<double2>> f64_c2r_kernel(const fftup_plan* P)
{
    return with_flag(P->inplaceI, [&](auto ip) { return kern(k_row_c2r<false, double2, ip()>, P->thrUW, P->ldsRowI); });
}
// non-R2C path: rows in one launch -- one instantiation per input type / output type / one-or-two-buffer form (1024 threads in place).
// (-p 1 plans read double planes whatever `kind` says: fuse_u8() is false for them, so their frames never have kind 2)
template <typename C> static Kern<RowR2CParamsT<C>> c2c_fwd_kernel(const fftup_plan* P, int kind)
{
    if constexpr (sizeof(scalar_t<C>) == 8) return kern(k_row_c2c_fwd<IN_F64, C, false>, P->thrW, P->ldsRowF);
    else return with_mode(P->half, kind, [&](auto m) {
        if (P->inplaceF) return kern(k_row_c2c_fwd<m(), C, true>, 1024, P->ldsRowF);
        return kern(k_row_c2c_fwd<m(), C, false>, P->thrW, P->ldsRowF);
    });
}
template <typename C> static Kern<RowC2RParamsT<C>> c2c_inv_kernel(const fftup_plan* P)
{
    if constexpr (sizeof(scalar_t<C>) == 8) return kern(k_row_c2c_inv<C, false, false>, P->thrUW, P->ldsRowI);
    else return with_flag(P->half, [&](auto h) {
        if (P->inplaceI) return kern(k_row_c2c_inv<C, h(), true>, 1024, P->ldsRowI);
        return kern(k_row_c2c_inv<C, h(), false>, P->thrUW, P->ldsRowI);
    });
}
// ... and rows or columns beyond the LDS in four steps: forward rows (input mode from the kind and the precision), inverse rows
// (output type from the precision), columns (dense, forward in place in S1, inverse S1 -> S2 with shift and guard)
template <typename C, int DIR, int MODE, int OUT> static FourKerns<C> four_kernels(const fftup_plan::Four& f)
{
    return {with_tile<16>(f.tka, [&](auto t) { return kern(k_row4_a<DIR, t(), MODE, C>, f.thrA, f.ldsA); }),
            with_tile<16>(f.tkb, [&](auto t) { return kern(k_row4_b<DIR, t(), OUT, C>, f.thrB, f.ldsB); })};
}
template <typename C> static FourKerns<C> four_fwd_kernels(const fftup_plan* P, int kind)
{
    if constexpr (sizeof(scalar_t<C>) == 8) return four_kernels<C, +1, IN_F64, OUT4_TILES>(P->fourF);
    else return with_mode(P->half, kind, [&](auto m) { return four_kernels<C, +1, m(), OUT4_TILES>(P->fourF); });
}
template <typename C> static FourKerns<C> four_inv_kernels(const fftup_plan* P)
{
    if constexpr (sizeof(scalar_t<C>) == 4) {
        if (P->half) return four_kernels<C, -1, IN4_TILES, OUT4_HALF>(P->fourI);
    }
    return four_kernels<C, -1, IN4_TILES, OUT4_DENSE>(P->fourI);
}
template <typename C> static FourKerns<C> four_col_kernels(const fftup_plan* P, bool inverse)
{
    return inverse ? four_kernels<C, -1, IN4_DENSE_SHIFT, OUT4_DENSE>(P->colI) : four_kernels<C, +1, IN4_DENSE, OUT4_DENSE>(P->colF);
}
// FFTUP_FLAG_DCT (kernels_dct.hpp)
static Kern<DctRowParams> dct_row_kernel(const fftup_plan* P, int kind)
{
    return with_mode(P->half, kind, [&](auto m) { return kern(k_dct_row<m()>, P->thrW, P->ldsRowF); });
}
static Kern<DctColParams> dct_col_kernel(const fftup_plan* P) { return with_tile(P->TK, [&](auto tk) { return kern(k_dct_col<tk()>, P->thrCol, P->ldsCol); }); }
static Kern<IdctRowParams> idct_row_kernel(const fftup_plan* P) { return with_flag(P->half, [&](auto h) { return kern(k_idct_row<h()>, P->thrUW, P->ldsRowI); }); }
// FFTUP_FLAG_DOWNSCALE, FFT mode (kernels_downscale.hpp; FFTUP_FLAG_ANY_SIZE: the instantiations with a Bluestein transform)
static Kern<DownRowParams> crop_row_kernel(const fftup_plan* P, int kind)
{
    return with_flag(P->bzW.L != 0, [&](auto bz) { return with_mode(P->half, kind, [&](auto m) { return kern(k_row_r2c_crop<m(), bz()>, P->thrW, P->ldsRowF); }); });
}
static Kern<DownColParams> crop_col_kernel(const fftup_plan* P)
{
    return with_flag(P->bzH.L || P->bzUH.L, [&](auto bz) { return with_tile(P->TK, [&](auto tk) { return kern(k_col_crop<tk(), bz()>, P->thrCol, P->ldsCol); }); });
}
// the resampling kernels (kernels_odd.hpp): FFTUP_FLAG_ODD_SIZE / fftup_plan_create_size; the forward rows of fftup_plan_create_view
// and the Bluestein forward rows of a size-generic plan
static Kern<OddRowParams> odd_row_kernel(const fftup_plan* P, int kind)
{
    return with_mode(P->half, kind, [&](auto m) { return kern(k_row_r2c_odd<m()>, P->thrW, P->ldsRowF); });
}
static Kern<OddColParams> odd_col_kernel(const fftup_plan* P) { return with_tile(P->TK, [&](auto tk) { return kern(k_col_odd<tk()>, P->thrCol, P->ldsCol); }); }
static Kern<OddC2RParams> odd_c2r_kernel(const fftup_plan* P) { return with_flag(P->half, [&](auto h) { return kern(k_row_c2r_odd<h()>, P->thrUW, P->ldsRowI); }); }
// the forward rows of a size-generic plan run the resampling row kernel when they are Bluestein transforms (what the attribute
// setter allows and what launch_frame_generic launches: both ask here)
static bool resampling_rows(const fftup_plan* P) { return P->family == Family::generic && P->bzW.L != 0; }
// fftup_plan_create_view (kernels_view.hpp)
static Kern<ViewColParams> view_col_kernel(const fftup_plan* P) { return with_tile(P->TK, [&](auto tk) { return kern(k_col_view<tk()>, P->thrCol, P->ldsCol); }); }
static Kern<ViewC2RParams> view_c2r_kernel(const fftup_plan* P) { return with_flag(P->half, [&](auto h) { return kern(k_row_view_c2r<h()>, P->thrUW, P->ldsRowI); }); }
// ... with FFTUP_FLAG_MIRROR (kernels_mirror.hpp): the same three passes on kernels of their own, sized like the view plans'
static Kern<MirrorRowParams> mirror_row_kernel(const fftup_plan* P, int kind)
{
    return with_mode(P->half, kind, [&](auto m) { return kern(k_row_r2c_mirror<m()>, P->thrW, P->ldsRowF); });
}
static Kern<MirrorColParams> mirror_col_kernel(const fftup_plan* P) { return with_tile(P->TK, [&](auto tk) { return kern(k_col_view_mirror<tk()>, P->thrCol, P->ldsCol); }); }
static Kern<MirrorC2RParams> mirror_c2r_kernel(const fftup_plan* P) { return with_flag(P->half, [&](auto h) { return kern(k_row_view_c2r_mirror<h()>, P->thrUW, P->ldsRowI); }); }
// ahead-of-time power-of-two plans (kernels_pow2.hpp, kernels_dswap.hpp: digit-swap column kernels, 4 KB of LDS per wave)
static Kern<RowR2CTParams> tuned_row_kernel(const fftup_plan* P, int kind)
{
    return with_mode(P->half, kind, [&](auto m) {
        switch (P->W) {
        case 512: return kern(k_row_r2c_t<512, m(), TUNED_TK>, 512 / 8, 0);
        case 1024: return kern(k_row_r2c_t<1024, m(), TUNED_TK>, 1024 / 8, 0);
        default: return kern(k_row_r2c_t<2048, m(), TUNED_TK>, 2048 / 8, 0);
        }
    });
}
static Kern<ColTParams> tuned_col_kernel(const fftup_plan* P)
{
    switch (P->H) {
    case 256: return kern(k_col_v<TUNED_TK, 256>, 128, 8192);
    case 512: return kern(k_col_v<TUNED_TK, 512>, 256, 16384);
    default: return kern(k_col_v<TUNED_TK, 1024>, 512, 32768);
    }
}
static Kern<RowC2RTParams> tuned_c2r_kernel(const fftup_plan* P)
{
    return with_flag(P->half, [&](auto h) {
        switch (P->uW) {
        case 1024: return kern(k_row_c2r_t<1024, h(), TUNED_TK, true>, 1024 / 8, 0);
        case 2048: return kern(k_row_c2r_t<2048, h(), TUNED_TK, true>, 2048 / 8, 0);
        default: return kern(k_row_c2r_t<4096, h(), TUNED_TK, true>, 4096 / 8, 0);
        }
    });
}
// ahead-of-time mixed-radix plans (kernels_mixed.hpp)
static Kern<RowR2CTParams> mixed_row_kernel(const fftup_plan* P, int kind)
{
    return with_mixed_cfg(P, [&](auto c) {
        using CFG = typename decltype(c)::type;
        return with_mode(P->half, kind, [&](auto m) { return kern(k_row_r2c_m<CFG, m()>, CFG::ROW_T, 0); });
    });
}
static Kern<ColTParams> mixed_col_kernel(const fftup_plan* P)
{
    return with_mixed_cfg(P, [&](auto c) { using CFG = typename decltype(c)::type; return kern(k_col_m<CFG>, 4 * CFG::COL_TPC, P->ldsCol); });
}
static Kern<RowC2RParams> mixed_c2r_kernel(const fftup_plan* P)
{
    return with_mixed_cfg(P, [&](auto c) {
        using CT = typename decltype(c)::type::CT;
        return with_flag(P->half, [&](auto h) { return kern(k_row_c2r_ct<CT, h()>, CT::T, P->ldsRowI); });
    });
}
// the fused C2R+sharpen kernel of the ahead-of-time plans: by the output width (power-of-two plans) or the configuration
template <class PL> static Kern<FusedParams> fused_kernel_of(const fftup_plan* P)
{
    return with_flag(P->half, [&](auto h) {
        if (P->u8out) return kern(k_c2r_sharpen_g<PL, h(), TUNED_TK, 2, 4, true>, PL::T, FusedGLds<PL>::TOTAL);
        return kern(k_c2r_sharpen_g<PL, h(), TUNED_TK>, PL::T, FusedGLds<PL>::TOTAL);
    });
}
static Kern<FusedParams> fused_kernel(const fftup_plan* P)
{
    if (P->family == Family::mixed_aot) return with_mixed_cfg(P, [&](auto c) { return fused_kernel_of<typename decltype(c)::type::FUSED>(P); });
    switch (P->uW) {
    case 1024: return fused_kernel_of<FusedPlanPow2<1024>>(P);
    case 2048: return fused_kernel_of<FusedPlanPow2<2048>>(P);
    default: return fused_kernel_of<FusedPlanPow2<4096>>(P);
    }
}

// ------------------------------------------------------------------------------------------------
// Allow every kernel THIS plan can launch its dynamic LDS (above 64 KB it is refused otherwise) -- the kernels the selectors hand
// to the frame functions below, for both input kinds; nothing else.  Kernels specialised at plan time are launched from their
// module, which asks for no such permission.  (Until the selectors existed, a FFTUP_FLAG_ANY_SIZE plan was also allowed the plain
// k_row_r2c / k_row_c2r / k_col beside the Bluestein forms it launches in their place; that surplus is gone.)
struct AllowLds {                     // what the selectors are asked with here; the first error is kept
    hipError_t err = hipSuccess;
    template <class... A, class... X> void operator()(const Kern<A...>& k, const X&...)
    {
        if (err == hipSuccess) err = hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds);
    }
    template <typename C> void operator()(const FourKerns<C>& k) { (*this)(k.a); (*this)(k.b); }
};
template <typename C> static void allow_columns(const fftup_plan* P, AllowLds& allow)
{
    if (P->colF.on) { allow(four_col_kernels<C>(P, false)); allow(four_col_kernels<C>(P, true)); }
    else columns_kernel<C>(P, allow);
}
template <typename C> static void allow_cplx(const fftup_plan* P, AllowLds& allow)
{
    for (int kind : {1, 2}) { if (P->fourF.on) allow(four_fwd_kernels<C>(P, kind)); else allow(c2c_fwd_kernel<C>(P, kind)); }
    allow_columns<C>(P, allow);
    if (P->fourI.on) allow(four_inv_kernels<C>(P)); else allow(c2c_inv_kernel<C>(P));
}
int kernels_set_attributes(fftup_plan* P)
{
    AllowLds allow;
    switch (P->family) {
    case Family::generic:
        for (int kind : {1, 2}) { if (resampling_rows(P)) allow(odd_row_kernel(P, kind)); else allow(generic_row_kernel(P, kind)); }
        allow_columns<float2>(P, allow);
        generic_c2r_kernel(P, allow);
        break;
    case Family::f64: allow(f64_row_kernel(P)); allow_columns<double2>(P, allow); allow(f64_c2r_kernel(P)); break;
    case Family::cplx: if (P->dbl) allow_cplx<double2>(P, allow); else allow_cplx<float2>(P, allow); break;
    case Family::dct: for (int kind : {1, 2}) allow(dct_row_kernel(P, kind)); allow(dct_col_kernel(P)); allow(idct_row_kernel(P)); break;
    case Family::down: for (int kind : {1, 2}) allow(crop_row_kernel(P, kind)); allow(crop_col_kernel(P)); generic_c2r_kernel(P, allow); break;
    case Family::odd: for (int kind : {1, 2}) allow(odd_row_kernel(P, kind)); allow(odd_col_kernel(P)); allow(odd_c2r_kernel(P)); break;
    case Family::view:
        if (P->mirror) { for (int kind : {1, 2}) allow(mirror_row_kernel(P, kind)); allow(mirror_col_kernel(P)); allow(mirror_c2r_kernel(P)); }
        else { for (int kind : {1, 2}) allow(odd_row_kernel(P, kind)); allow(view_col_kernel(P)); allow(view_c2r_kernel(P)); }
        break;
    case Family::tuned: allow(tuned_col_kernel(P)); allow(fused_kernel(P)); break;          // (rows: static LDS)
    case Family::mixed_aot: allow(mixed_col_kernel(P)); allow(mixed_c2r_kernel(P)); allow(fused_kernel(P)); break;
    case Family::mixed_jit:           // (a plan-time plan without a row factorization runs the size-generic row kernel)
        if (P->jit->choice.row_kind == 2) for (int kind : {1, 2}) allow(generic_row_kernel(P, kind));
        break;
    }
    if (allow.err != hipSuccess) return fail(FFTUP_E_HIP, std::string("hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize): ") + hipGetErrorString(allow.err));
    return FFTUP_OK;
}

// ------------------------------------------------------------------------------------------------
// the two host loops of the reference as kernels (VR:1636-1685, VR:1708-1748)
void launch_unpack_from(fftup_plan* P, const uint8_t* rgb, size_t row_stride_bytes, void* planes, hipStream_t st)
{
    dim3 grid((P->W + 255) / 256, P->H);
    if (P->dbl)
        hipLaunchKernelGGL(k_unpack_u8_f64, grid, dim3(256), 0, st, rgb, (long)row_stride_bytes, (double*)planes,
                           (int)P->W, (int)P->H, (long)P->in_plane_stride);
    else if (P->half)
        hipLaunchKernelGGL(k_unpack_u8<true>, grid, dim3(256), 0, st, rgb, (long)row_stride_bytes, planes,
                           (int)P->W, (int)P->H, (long)P->in_plane_stride);
    else
        hipLaunchKernelGGL(k_unpack_u8<false>, grid, dim3(256), 0, st, rgb, (long)row_stride_bytes, planes,
                           (int)P->W, (int)P->H, (long)P->in_plane_stride);
}
void launch_unpack(fftup_plan* P, uint32_t slot, hipStream_t st) { launch_unpack_from(P, P->in_u8[slot], (size_t)3 * P->W, P->in_planar[slot], st); }

void launch_pack(fftup_plan* P, uint32_t slot, uint8_t* dst, hipStream_t st)
{
    dim3 grid(P->dbl ? (P->uW + 255) / 256 : (P->uW + 1023) / 1024, P->uH);      // (float / half: four pixels per thread)
    const int wrap = (P->cfg.flags & FFTUP_FLAG_U8_WRAP) ? 1 : 0;
    if (P->dbl) hipLaunchKernelGGL(k_pack_u8_f64, grid, dim3(256), 0, st, (const double*)P->out[slot], dst, (int)P->uW, (int)P->uH, wrap);
    else if (P->half) hipLaunchKernelGGL(k_pack_u8<true>, grid, dim3(256), 0, st, P->out[slot], dst, (int)P->uW, (int)P->uH, wrap);
    else hipLaunchKernelGGL(k_pack_u8<false>, grid, dim3(256), 0, st, P->out[slot], dst, (int)P->uW, (int)P->uH, wrap);
}

// fftup_execute_device: the conversion of launch_pack from a lane's scratch planes into rows of the caller's stride
void launch_pack_to(fftup_plan* P, const void* planes, uint8_t* rgb, size_t row_stride_bytes, hipStream_t st)
{
    dim3 grid(P->dbl ? (P->uW + 255) / 256 : (P->uW + 1023) / 1024, P->uH);
    const int wrap = (P->cfg.flags & FFTUP_FLAG_U8_WRAP) ? 1 : 0;
    if (P->dbl) hipLaunchKernelGGL(k_pack_u8_f64_strided, grid, dim3(256), 0, st, (const double*)planes, rgb, (long)row_stride_bytes, (int)P->uW, (int)P->uH, wrap);
    else if (P->half) hipLaunchKernelGGL(k_pack_u8_strided<true>, grid, dim3(256), 0, st, planes, rgb, (long)row_stride_bytes, (int)P->uW, (int)P->uH, wrap);
    else hipLaunchKernelGGL(k_pack_u8_strided<false>, grid, dim3(256), 0, st, planes, rgb, (long)row_stride_bytes, (int)P->uW, (int)P->uH, wrap);
}

void launch_copy_rows(const void* src, size_t src_row, size_t src_plane, void* dst, size_t dst_row, size_t dst_plane,
                      size_t row_bytes, uint32_t rows, uint32_t planes, int gran, hipStream_t st)
{
    CopyRowsParams p{};
    p.src = (const uint8_t*)src; p.dst = (uint8_t*)dst; p.src_row = (long)src_row; p.src_plane = (long)src_plane;
    p.dst_row = (long)dst_row; p.dst_plane = (long)dst_plane; p.row_bytes = (long)row_bytes;
    const dim3 grid((unsigned)((row_bytes / 16 + 2 + 255) / 256), rows, planes);
    switch (gran) {
    case 8: hipLaunchKernelGGL(k_copy_rows<8>, grid, dim3(256), 0, st, p); break;
    case 4: hipLaunchKernelGGL(k_copy_rows<4>, grid, dim3(256), 0, st, p); break;
    case 2: hipLaunchKernelGGL(k_copy_rows<2>, grid, dim3(256), 0, st, p); break;
    default: hipLaunchKernelGGL(k_copy_rows<1>, grid, dim3(256), 0, st, p); break;
    }
}

// (test builds, FFTUP_EXPERIMENT planes=1: the row and column passes of the power-of-two plans on the first colour plane only --
// what one plane's pass costs alone on the whole GPU, the start-up a frame pipelined by planes cannot hide; results invalid)
static unsigned pass_planes()
{
    const char* e = fftup_jit::experiment("planes");
    return e ? (unsigned)std::max(1, std::min(3, atoi(e))) : 3u;
}

// workgroups of the fused C2R+sharpen kernel.  Planes: strips in linear order over the 3 uH/2 row pairs.  Fused 8-bit store:
// strips per plane, the three planes' strips of the same rows 8 workgroups apart, rows of 8 strips (k_c2r_sharpen_g, OUT_U8)
static unsigned fused_grid(const fftup_plan* P, int pairs_per_strip)
{
    const int ppp = (int)P->uH / 2;
    if (P->u8out) return (unsigned)(((ppp + pairs_per_strip - 1) / pairs_per_strip + 7) / 8 * 24);
    return (unsigned)((3 * ppp + pairs_per_strip - 1) / pairs_per_strip);
}
static FusedParams fused_params(const fftup_plan* P, const Frame& f)
{
    FusedParams p{};
    p.S1 = f.S1; p.odd_delta = (unsigned)(f.S2 - f.S1);
    if (P->U == 1) { p.S1 = f.S2; p.odd_delta = 0; }      // half-integer factor: one buffer with all rows (k_col_pad)
    p.out = f.out; p.tw = P->twUW; p.uH = (int)P->uH; p.NT = P->NT;
    p.pairs_per_strip = P->pairs_per_strip; p.upsq = P->upsq; p.coef = P->coef;
    p.u8_wrap = (P->cfg.flags & FFTUP_FLAG_U8_WRAP) ? 1 : 0;
    return p;
}

static bool fast_sharpen_ok(const fftup_plan* P) { return !P->dbl && P->uW % 256 == 0 && P->uH % 16 == 0; }

static void launch_sharpen_fast(const fftup_plan* P, const Frame& f)
{
    SharpenTParams p{};
    p.R = f.R; p.out = f.out; p.uW = (int)P->uW; p.uH = (int)P->uH; p.upsq = f.upsq; p.coef = P->coef;
    dim3 grid(P->uW / 256, P->uH / 16, 3), block(64, 4);
    if (P->half) hipLaunchKernelGGL((k_sharpen_t<true, 4>), grid, block, 0, f.st, p);
    else hipLaunchKernelGGL((k_sharpen_t<false, 4>), grid, block, 0, f.st, p);
}

// the sharpen pass of an unfused fp32 / fp16 plan: R -> the frame's output image
static void launch_sharpen(const fftup_plan* P, const Frame& f)
{
    if (fast_sharpen_ok(P)) { launch_sharpen_fast(P, f); return; }
    SharpenParams p{};
    p.R = f.R; p.out = f.out; p.uW = (int)P->uW; p.uH = (int)P->uH; p.upsq = f.upsq; p.coef = P->coef;
    dim3 grid((P->uW + 1023) / 1024, P->uH, 3), block(256);      // (four pixels per thread; a width of 2 gave an empty grid until round 5)
    if (P->half) hipLaunchKernelGGL(k_sharpen<true>, grid, block, 0, f.st, p);
    else hipLaunchKernelGGL(k_sharpen<false>, grid, block, 0, f.st, p);
}

// the end of every frame function: the first failing launch of the frame wins (`jit`: launches from a run-time specialised code
// object report their errors directly)
static int frame_status(hipError_t jit = hipSuccess)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = jit;
    if (e != hipSuccess) return fail(FFTUP_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return FFTUP_OK;
}

// The frame of the families with four launches on fp32 / fp16 data: forward rows, columns, inverse rows into R, sharpen
template <class Rows, class Cols, class Inv>
static int launch_four_passes(const fftup_plan* P, const Frame& f, Pass pass, Rows rows, Cols cols, Inv inv)
{
    if (runs(pass, Pass::rows)) rows(P, f);
    if (runs(pass, Pass::columns)) cols(P, f);
    if (runs(pass, Pass::inverse)) inv(P, f);
    if (runs(pass, Pass::sharpen)) launch_sharpen(P, f);
    return frame_status();
}

// ---- FFTUP_FLAG_DCT: DCT-II rows -> DCT-II columns, zero-pad, DCT-III columns -> DCT-III rows -> sharpen (kernels_dct.hpp)
static void dct_rows(const fftup_plan* P, const Frame& f)
{
    DctRowParams p{};
    p.S1 = (float*)f.S1; p.tw = P->twW; p.rot = P->rotW; p.plan = P->planW; p.W = (int)P->W; p.H = (int)P->H;
    set_in(f, p);
    launch(dct_row_kernel(P, f.kind), dim3(P->H / 2, 3), f.st, p);
}
static void dct_cols(const fftup_plan* P, const Frame& f)
{
    DctColParams p{};
    p.S1 = (const float*)f.S1; p.S2 = (float*)f.S2;
    p.twH = P->twH; p.twUH = P->twUH; p.rotH = P->rotH; p.rotUH = P->rotUH; p.planH = P->planH; p.planUH = P->planUH;
    p.W = (int)P->W; p.H = (int)P->H; p.uH = (int)P->uH; p.inv_norm = (float)(1.0 / (double)P->H);
    launch(dct_col_kernel(P), dim3((P->W / 2 + P->TK - 1) / P->TK, 3), f.st, p);
}
static void dct_inv(const fftup_plan* P, const Frame& f)
{
    IdctRowParams p{};
    p.S2 = (const float*)f.S2; p.R = f.R; p.tw = P->twUW; p.rot = P->rotUW; p.plan = P->planUW;
    p.W = (int)P->W; p.uW = (int)P->uW; p.uH = (int)P->uH;
    p.inv_norm = (float)(1.0 / ((double)P->W * (double)P->upsq));
    launch(idct_row_kernel(P), dim3(P->uH / 2, 3), f.st, p);
}

// ---- FFTUP_FLAG_DOWNSCALE (FFT mode): row R2C keeping kx <= uW/2 -> column forward / crop / inverse -> the upscale path's C2R with
// W := uW and no read guard -> sharpen (kernels_downscale.hpp)
static void down_rows(const fftup_plan* P, const Frame& f)
{
    DownRowParams p{};
    p.S1 = f.S1; p.tw = P->twW; p.plan = P->planW; p.W = (int)P->W; p.H = (int)P->H;
    p.TK = P->TK; p.NT = P->NT; p.h = (int)P->uW / 2; p.bz = P->bzW;
    set_in(f, p);
    launch(crop_row_kernel(P, f.kind), dim3(P->H / 2, 3), f.st, p);
}
static void down_cols(const fftup_plan* P, const Frame& f)
{
    DownColParams p{};
    p.S1 = f.S1; p.S2 = f.S2; p.twH = P->twH; p.twUH = P->twUH; p.planH = P->planH; p.planUH = P->planUH;
    p.H = (int)P->H; p.uH = (int)P->uH; p.NT = P->NT; p.ncols = P->ncols; p.inv_norm = 1.0f / (float)P->uH;
    p.bzH = P->bzH; p.bzUH = P->bzUH;
    launch(crop_col_kernel(P), dim3(P->NT, 3), f.st, p);
}
static void down_inv(const fftup_plan* P, const Frame& f)
{
    // W := uW: every bin k <= uW/2 is read; the empty guard [0, 0); the folded Nyquist bin is real, so the kernel's two writes
    // of a[uW/2] (from k and from uW - k) store the same value
    RowC2RParams p{};
    p.S2 = f.S2; p.R = f.R; p.tw = P->twUW; p.plan = P->planUW; p.W = (int)P->uW; p.uW = (int)P->uW;
    p.uH = (int)P->uH; p.TK = P->TK; p.NT = P->NT; p.zlx = 0; p.zrx = 0; p.inv_norm = 1.0f / (float)P->uW; p.poly = 0;
    generic_c2r_kernel(P, [&](auto k, const auto&... z) { launch(k, dim3(P->uH / 2, 3), f.st, p, z...); });
}

// ---- FFTUP_FLAG_ODD_SIZE with an odd length: row R2C keeping kx <= min(W, uW)/2 -> column forward / bin map / inverse -> row C2R ->
// sharpen (kernels_odd.hpp).  Up, down or -u 1; (rows + 1) / 2 workgroups per plane, the last one with a single row when odd.
// Plans of fftup_plan_create_size run the same four launches, each axis with its own direction, centre-aligned ones with phase tables.
// fftup_plan_create_view runs the same row R2C keeping kx <= kmax_x, without fold or phase table.  Size-generic plans with
// Bluestein forward rows run it too: kmax = W/2 (uW >= W), no fold, P->phW == nullptr.
static void odd_rows(const fftup_plan* P, const Frame& f)
{
    const bool view = P->family == Family::view;
    OddRowParams p{};
    p.S1 = f.S1; p.tw = P->twW; p.plan = P->planW; p.W = (int)P->W; p.H = (int)P->H;
    p.TK = P->TK; p.NT = f.NT; p.bz = P->bzW;
    p.kmax = view ? f.vx.kmax : (int)std::min(P->W, P->uW) / 2;
    p.fold = (!view && P->uW < P->W && !(P->uW & 1)) ? 1 : 0;
    p.ph = view ? nullptr : P->phW;
    set_in(f, p);
    launch(odd_row_kernel(P, f.kind), dim3((P->H + 1) / 2, 3), f.st, p);
}
static void odd_cols(const fftup_plan* P, const Frame& f)
{
    OddColParams p{};
    p.S1 = f.S1; p.S2 = f.S2; p.twH = P->twH; p.twUH = P->twUH; p.planH = P->planH; p.planUH = P->planUH;
    p.H = (int)P->H; p.uH = (int)P->uH; p.NT = P->NT; p.ncols = P->ncols; p.inv_norm = 1.0f / (float)P->uH;
    p.bzH = P->bzH; p.bzUH = P->bzUH; p.ph = P->phH;
    launch(odd_col_kernel(P), dim3(P->NT, 3), f.st, p);
}
static void odd_inv(const fftup_plan* P, const Frame& f)
{
    OddC2RParams p{};
    p.S2 = f.S2; p.R = f.R; p.tw = P->twUW; p.plan = P->planUW; p.uW = (int)P->uW; p.uH = (int)P->uH;
    p.TK = P->TK; p.NT = P->NT; p.kmax = (int)std::min(P->W, P->uW) / 2; p.halve = (P->uW > P->W && !(P->W & 1)) ? 1 : 0; p.inv_norm = 1.0f / (float)P->uW;
    p.bz = P->bzUW;
    launch(odd_c2r_kernel(P), dim3((P->uH + 1) / 2, 3), f.st, p);
}

// ---- fftup_plan_create_view: the odd-size plans' row R2C -> column forward / signed bins / chirp-z to uH points -> two spectrum
// rows / chirp-z to uW points -> sharpen (kernels_view.hpp)
// (the length, its radix list and roots are the plan's; kmax and the three tables the frame's)
static CztPlan czt_plan(const fftup_plan::ViewAxis& a, const ViewTables& t, uint32_t M)
{
    CztPlan z{};
    z.L = (int32_t)a.L; z.K = 2 * t.kmax + 1; z.M = (int32_t)M; z.plan = a.planL; z.tw = a.tw; z.pre = t.pre; z.post = t.post; z.bhat = t.bhat;
    return z;
}
static void view_cols(const fftup_plan* P, const Frame& f)
{
    ViewColParams p{};
    p.S1 = f.S1; p.S2 = f.S2; p.twH = P->twH; p.planH = P->planH;
    p.H = (int)P->H; p.uH = (int)P->uH; p.NT = f.NT; p.ncols = f.ncols; p.kmax = f.vy.kmax; p.bzH = P->bzH; p.z = czt_plan(P->vy, f.vy, P->uH);
    launch(view_col_kernel(P), dim3(f.NT, 3), f.st, p);
}
static void view_inv(const fftup_plan* P, const Frame& f)
{
    ViewC2RParams p{};
    p.S2 = f.S2; p.R = f.R; p.uW = (int)P->uW; p.uH = (int)P->uH;
    p.TK = P->TK; p.NT = f.NT; p.kmax = f.vx.kmax; p.z = czt_plan(P->vx, f.vx, P->uW);
    launch(view_c2r_kernel(P), dim3((P->uH + 1) / 2, 3), f.st, p);
}

// ---- ... with FFTUP_FLAG_MIRROR: reordered row R2C (unphased half spectra) -> column DCT-II through a transform of H points /
// Z = 2 C[|f|] / chirp-z over the period 2H -> cosine coefficients of two rows / chirp-z over the period 2W -> sharpen
// (kernels_mirror.hpp; the tables: mirror_tables.hpp)
static void mirror_rows(const fftup_plan* P, const Frame& f)
{
    MirrorRowParams p{};
    p.S1 = f.S1; p.tw = P->twW; p.plan = P->planW; p.W = (int)P->W; p.H = (int)P->H;
    p.TK = P->TK; p.NT = f.NT; p.ncols = f.ncols; p.bz = P->bzW;
    set_in(f, p);
    launch(mirror_row_kernel(P, f.kind), dim3((P->H + 1) / 2, 3), f.st, p);
}
static void mirror_cols(const fftup_plan* P, const Frame& f)
{
    MirrorColParams p{};
    p.S1 = f.S1; p.S2 = f.S2; p.twH = P->twH; p.planH = P->planH;
    p.H = (int)P->H; p.uH = (int)P->uH; p.NT = f.NT; p.ncols = f.ncols; p.kmax = f.vy.kmax; p.bzH = P->bzH; p.z = czt_plan(P->vy, f.vy, P->uH);
    p.rot = P->rotH;
    launch(mirror_col_kernel(P), dim3(f.NT, 3), f.st, p);
}
static void mirror_inv(const fftup_plan* P, const Frame& f)
{
    MirrorC2RParams p{};
    p.S2 = f.S2; p.R = f.R; p.W = (int)P->W; p.uW = (int)P->uW; p.uH = (int)P->uH;
    p.TK = P->TK; p.NT = f.NT; p.kmax = f.vx.kmax; p.z = czt_plan(P->vx, f.vx, P->uW); p.rot = P->rotW;
    launch(mirror_c2r_kernel(P), dim3((P->uH + 1) / 2, 3), f.st, p);
}

// ---- four-step transforms (k_row4_a / k_row4_b): both passes of one
template <typename C> static void launch_four(const FourKerns<C>& k, const fftup_plan::Four& f, const Row4Params<C>& q, int rows, hipStream_t st)
{
    launch(k.a, dim3(rows, f.n2 / f.tka, 3), st, q);
    launch(k.b, dim3(rows, f.n1 / f.tkb, 3), st, q);
}
// the column pass of the size-generic plans on C: in LDS, or -- columns longer than the LDS -- in four steps, forward in place
// in S1 (tiles of one column = dense columns), inverse S1 -> S2 with shift and guard
template <typename C> static void launch_columns(const fftup_plan* P, const Frame& f)
{
    using S = scalar_t<C>;
    if (!P->colF.on) {
        ColParamsT<C> p{};
        p.S1 = (const C*)f.S1; p.S2 = (C*)f.S2; p.twH = (const C*)P->twH; p.twUH = (const C*)P->twUH;
        p.planH = P->planH; p.planUH = P->planUH;
        p.W = (int)P->W; p.H = (int)P->H; p.uH = (int)P->uH; p.NT = P->NT; p.ncols = P->ncols; p.zly = P->zly; p.zry = P->zry;
        p.inv_norm = (S)(1.0 / (double)P->uH);
        columns_kernel<C>(P, [&](auto k, const auto&... z) { launch(k, dim3(P->NT, 3), f.st, p, z...); });
        return;
    }
    Row4Params<C> q{};
    const fftup_plan::Four &s = P->colF, &g = P->colI;
    q.spec = (const C*)f.S1; q.T = (C*)f.T4; q.R = f.S1;
    q.tw1 = (const C*)P->colFtw.tw1; q.tw2 = (const C*)P->colFtw.tw2; q.twN = (const C*)P->twH; q.plan1 = s.p1; q.plan2 = s.p2;
    q.N = (int)P->H; q.N1 = s.n1; q.N2 = s.n2; q.rows = P->ncols; q.W = (int)P->H; q.TK = 1; q.NT = P->ncols; q.inv_norm = (S)1;
    launch_four(four_col_kernels<C>(P, false), s, q, P->ncols, f.st);
    q.R = f.S2; q.tw1 = (const C*)P->colItw.tw1; q.tw2 = (const C*)P->colItw.tw2; q.twN = (const C*)P->twUH; q.plan1 = g.p1; q.plan2 = g.p2;
    q.N = (int)P->uH; q.N1 = g.n1; q.N2 = g.n2; q.zlx = P->zly; q.zrx = P->zry; q.inv_norm = (S)(1.0 / (double)P->uH);
    launch_four(four_col_kernels<C>(P, true), g, q, P->ncols, f.st);
}

// ---- -p 1: the size-generic kernels instantiated on double2 + the double sharpen
static int launch_frame_f64(const fftup_plan* P, const Frame& f, Pass pass)
{
    if (runs(pass, Pass::rows)) {
        RowR2CParamsT<double2> p{};
        p.S1 = (double2*)f.S1; p.tw = (const double2*)P->twW; p.plan = P->planW; p.W = (int)P->W; p.H = (int)P->H;
        p.TK = P->TK; p.NT = P->NT;
        set_in(f, p);
        launch(f64_row_kernel(P), dim3(P->H / 2, 3), f.st, p);
    }
    if (runs(pass, Pass::columns)) launch_columns<double2>(P, f);
    if (runs(pass, Pass::inverse)) {
        RowC2RParamsT<double2> p{};
        p.S1 = (const double2*)f.S1; p.S2 = (const double2*)f.S2; p.R = f.R; p.tw = (const double2*)P->twUW; p.plan = P->planUW;
        p.W = (int)P->W; p.uW = (int)P->uW; p.uH = (int)P->uH; p.TK = P->TK; p.NT = P->NT; p.zlx = P->zlx; p.zrx = P->zrx;
        p.inv_norm = 1.0 / (double)P->uW; p.poly = P->poly;
        launch(f64_c2r_kernel(P), dim3(P->uH / 2, 3), f.st, p);
    }
    if (runs(pass, Pass::sharpen)) {
        SharpenParams p{};
        p.R = f.R; p.out = f.out; p.uW = (int)P->uW; p.uH = (int)P->uH; p.upsq = P->upsq; p.coef = P->coef;
        const dim3 sgrid((P->uW + 511) / 512, (P->uH + SHARPEN_F64_RPT - 1) / SHARPEN_F64_RPT, 3);
        const char* ex = fftup_jit::experiment("f64_exact_sharpen");          // (test builds: IEEE divisions and root)
        if (ex && atoi(ex)) {
            if (P->uW % 2 == 0) hipLaunchKernelGGL((k_sharpen_f64<true, true>), sgrid, dim3(64, 4), 0, f.st, p);
            else hipLaunchKernelGGL((k_sharpen_f64<false, true>), sgrid, dim3(64, 4), 0, f.st, p);
        }
        else if (P->uW % 2 == 0) hipLaunchKernelGGL(k_sharpen_f64<true>, sgrid, dim3(64, 4), 0, f.st, p);
        else hipLaunchKernelGGL(k_sharpen_f64<false>, sgrid, dim3(64, 4), 0, f.st, p);
    }
    return frame_status();
}

// ---- non-R2C path: four launches of size-generic kernels on complex data; rows beyond one LDS buffer in four
// steps through HBM
template <typename C> static int launch_frame_cplx(const fftup_plan* P, const Frame& f, Pass pass)
{
    using S = scalar_t<C>;
    if (runs(pass, Pass::rows) && P->fourF.on) {
        Row4Params<C> q{};
        const fftup_plan::Four& s = P->fourF;
        q.T = (C*)f.T4; q.S1 = (C*)f.S1; q.tw1 = (const C*)P->fourFtw.tw1; q.tw2 = (const C*)P->fourFtw.tw2; q.twN = (const C*)P->twW;
        q.plan1 = s.p1; q.plan2 = s.p2; q.N = (int)P->W; q.N1 = s.n1; q.N2 = s.n2; q.rows = (int)P->H; q.W = (int)P->W; q.TK = P->TK; q.NT = P->NT;
        set_in(f, q);
        launch_four(four_fwd_kernels<C>(P, f.kind), s, q, (int)P->H, f.st);
    } else if (runs(pass, Pass::rows)) {
        RowR2CParamsT<C> p{};
        p.S1 = (C*)f.S1; p.tw = (const C*)P->twW; p.plan = P->planW; p.W = (int)P->W; p.H = (int)P->H;
        p.TK = P->TK; p.NT = P->NT;
        set_in(f, p);
        launch(c2c_fwd_kernel<C>(P, f.kind), dim3(P->H, 3), f.st, p);
    }
    if (runs(pass, Pass::columns)) launch_columns<C>(P, f);
    if (runs(pass, Pass::inverse)) {
        if (P->fourI.on) {
            Row4Params<C> q{};
            const fftup_plan::Four& s = P->fourI;
            q.spec = (const C*)f.S2; q.T = (C*)f.T4; q.R = f.R;
            q.tw1 = (const C*)P->fourItw.tw1; q.tw2 = (const C*)P->fourItw.tw2; q.twN = (const C*)P->twUW; q.plan1 = s.p1; q.plan2 = s.p2;
            q.N = (int)P->uW; q.N1 = s.n1; q.N2 = s.n2; q.rows = (int)P->uH; q.W = (int)P->W; q.TK = P->TK; q.NT = P->NT; q.zlx = P->zlx; q.zrx = P->zrx;
            q.inv_norm = (S)(1.0 / (double)P->uW);
            launch_four(four_inv_kernels<C>(P), s, q, (int)P->uH, f.st);
        } else {
            RowC2RParamsT<C> p{};
            p.S2 = (const C*)f.S2; p.R = f.R; p.tw = (const C*)P->twUW; p.plan = P->planUW;
            p.W = (int)P->W; p.uW = (int)P->uW; p.uH = (int)P->uH; p.TK = P->TK; p.NT = P->NT; p.zlx = P->zlx; p.zrx = P->zrx;
            p.inv_norm = (S)(1.0 / (double)P->uW);
            launch(c2c_inv_kernel<C>(P), dim3(P->uH, 3), f.st, p);
        }
    }
    if (runs(pass, Pass::sharpen)) {
        SharpenParams p{};
        p.R = f.R; p.out = f.out; p.uW = (int)P->uW; p.uH = (int)P->uH; p.upsq = P->upsq; p.coef = P->coef;
        const dim3 grid((P->uW + 255) / 256, P->uH, 3);
        bool done = false;
        if constexpr (sizeof(S) == 4) {
            if (P->half) { hipLaunchKernelGGL((k_sharpen_c<C, true>), grid, dim3(256), 0, f.st, p); done = true; }
        }
        if (!done) hipLaunchKernelGGL((k_sharpen_c<C>), grid, dim3(256), 0, f.st, p);
    }
    return frame_status();
}

// ---- ahead-of-time plans: power-of-two sizes (kernels_pow2.hpp, kernels_dswap.hpp) and the two mixed-radix configurations
// (kernels_mixed.hpp).  Fused C2R+sharpen unless FFTUP_FLAG_UNFUSED_SHARPEN; Pass::presharpen_tap runs the stand-alone C2R of a fused plan
static int launch_frame_tuned(const fftup_plan* P, const Frame& f, Pass pass)
{
    if (runs(pass, Pass::rows)) {
        RowR2CTParams p{};
        p.S1 = f.S1; p.tw = P->twW; p.H = (int)P->H; p.NT = P->NT;
        set_in(f, p);
        launch(tuned_row_kernel(P, f.kind), dim3(P->H / 2, pass_planes()), f.st, p);
    }
    if (runs(pass, Pass::columns)) {
        ColTParams p{};
        p.S1 = f.S1; p.S2 = f.S2; p.twH = P->twH; p.twUH = P->twUH; p.W = (int)P->W; p.NT = P->NT;
        p.zly = P->zly; p.zry = P->zry;
        launch(tuned_col_kernel(P), dim3(P->NT, pass_planes()), f.st, p);
    }
    if (runs(pass, Pass::inverse) && P->fused) {
        const FusedParams p = fused_params(P, f);
        launch(fused_kernel(P), dim3(fused_grid(P, p.pairs_per_strip)), f.st, p);
    } else if (runs(pass, Pass::inverse) || pass == Pass::presharpen_tap) {
        RowC2RTParams p{};
        p.S1 = f.S1; p.S2 = f.S2; p.R = f.R; p.tw = P->twUW; p.uH = (int)P->uH; p.NT = P->NT;
        launch(tuned_c2r_kernel(P), dim3(P->uH / 2, 3), f.st, p);
    }
    if (runs(pass, Pass::sharpen) && !P->fused) launch_sharpen_fast(P, f);
    return frame_status();
}

// ---- the size-generic R2C plans on fp32 / fp16 data (kernels_generic.hpp; FFTUP_FLAG_ANY_SIZE: kernels_bluestein.hpp, odd_rows) and the
// mixed-radix plans: ahead of time (kernels_mixed.hpp) or specialised at plan time -- those are launched from P->jit as it is NOW
// (the tuner swaps it after plan creation)
static int launch_frame_generic(const fftup_plan* P, const Frame& f, Pass pass)
{
    const bool jit = P->family == Family::mixed_jit, aot = P->family == Family::mixed_aot;
    hipError_t jerr = hipSuccess;
    auto keep_first = [&](hipError_t e) { if (jerr == hipSuccess) jerr = e; };       // (later launches must not mask an earlier failure)
    if (runs(pass, Pass::rows)) {
        const dim3 grid(P->H / 2, 3);
        if (resampling_rows(P)) odd_rows(P, f);
        else if (aot || (jit && P->jit->choice.row_kind != 2)) {
            RowR2CTParams q{};
            q.S1 = f.S1; q.tw = P->twW; q.H = (int)P->H; q.NT = P->NT;
            set_in(f, q);
            if (aot) launch(mixed_row_kernel(P, f.kind), grid, f.st, q);
            else keep_first(fftup_jit::launch(P->jit->fn[f.kind == 2 ? fftup_jit::K_ROW_U8 : fftup_jit::K_ROW_PLANAR], grid, dim3(P->jit->choice.row_block), 0, f.st, q));
        } else {
            RowR2CParams p{};
            p.S1 = f.S1; p.tw = P->twW; p.plan = P->planW; p.W = (int)P->W; p.H = (int)P->H;
            p.TK = P->TK; p.NT = P->NT;
            set_in(f, p);
            launch(generic_row_kernel(P, f.kind), grid, f.st, p);
        }
    }
    if (runs(pass, Pass::columns) && (jit || aot)) {
        ColTParams q{};
        q.S1 = f.S1; q.S2 = f.S2; q.twH = P->twH; q.twUH = P->twUH; q.W = (int)P->W; q.NT = P->NT;
        q.zly = P->zly; q.zry = P->zry;
        if (jit) {
            const auto& ch = P->jit->choice;
            const dim3 jgrid(P->NT * (ch.col_kind >= 3 ? 4 / ch.col_cols : 1), 3);        // (long columns: two per workgroup)
            keep_first(fftup_jit::launch(P->jit->fn[fftup_jit::K_COL], jgrid, dim3(ch.col_block), P->ldsCol, f.st, q));
        }
        else launch(mixed_col_kernel(P), dim3(P->NT, 3), f.st, q);
    }
    else if (runs(pass, Pass::columns)) launch_columns<float2>(P, f);
    if (runs(pass, Pass::inverse) && P->fused) {
        const FusedParams fp = fused_params(P, f);
        const dim3 grid(fused_grid(P, fp.pairs_per_strip));
        if (jit) keep_first(fftup_jit::launch(P->jit->fn[fftup_jit::K_FUSED], grid, dim3(P->jit->choice.fused_t), P->jit->choice.fused_lds, f.st, fp));
        else launch(fused_kernel(P), grid, f.st, fp);                    // (only the mixed plans are fused on this path)
    } else if (runs(pass, Pass::inverse) || pass == Pass::presharpen_tap) {
        RowC2RParams p{};
        p.S1 = f.S1; p.S2 = f.S2; p.R = f.R; p.tw = P->twUW; p.plan = P->planUW; p.W = (int)P->W; p.uW = (int)P->uW;
        p.uH = (int)P->uH; p.TK = P->TK; p.NT = P->NT; p.zlx = P->zlx; p.zrx = P->zrx;
        p.inv_norm = 1.0f / (float)P->uW; p.poly = P->poly && !P->mixed;
        const dim3 grid(P->uH / 2, 3);
        if (jit) {
            if (P->U == 1) p.S1 = p.S2;                              // half-integer factor: all rows in S2
            keep_first(fftup_jit::launch(P->jit->fn[fftup_jit::K_C2R_CT], grid, dim3(P->jit->choice.ct_t), P->ldsRowI, f.st, p));
        }
        else if (aot) launch(mixed_c2r_kernel(P), grid, f.st, p);
        else generic_c2r_kernel(P, [&](auto k, const auto&... z) { launch(k, grid, f.st, p, z...); });
    }
    if (runs(pass, Pass::sharpen) && !P->fused) launch_sharpen(P, f);
    return frame_status(jerr);
}

static int launch_family(const fftup_plan* P, const Frame& f, Pass pass)
{
    switch (P->family) {
    case Family::cplx: return P->dbl ? launch_frame_cplx<double2>(P, f, pass) : launch_frame_cplx<float2>(P, f, pass);
    case Family::f64: return launch_frame_f64(P, f, pass);
    case Family::dct: return launch_four_passes(P, f, pass, dct_rows, dct_cols, dct_inv);
    case Family::down: return launch_four_passes(P, f, pass, down_rows, down_cols, down_inv);
    case Family::odd: return launch_four_passes(P, f, pass, odd_rows, odd_cols, odd_inv);
    case Family::view:
        if (P->mirror) return launch_four_passes(P, f, pass, mirror_rows, mirror_cols, mirror_inv);
        return launch_four_passes(P, f, pass, odd_rows, view_cols, view_inv);
    case Family::tuned: return launch_frame_tuned(P, f, pass);
    case Family::generic: case Family::mixed_aot: case Family::mixed_jit: break;
    }
    return launch_frame_generic(P, f, pass);
}
// ---- a frame with a view of its own (fftup_execute_device_views): what view_apply derives on the host for the plan's view, here
// for this frame -- kmax per axis as kmax_of / mirror_kmax_of, the columns kept, the sharpen constant of its spans -- and the
// tables from k_view_tables, enqueued on the lane's stream ahead of the frame's kernels into the lane's own set (view_frames_prepare
// made it).  An axis whose span is the one the lane's chirp tables were built for rebuilds `pre` alone.  No event, no copy, no
// host synchronisation: the lane's next frame rebuilds the tables behind this frame's last reader.
static Kern<ViewTabParams> view_tables_kernel(const fftup_plan* P)
{
    return kern(k_view_tables, VT_THREADS, sizeof(double2) * (size_t)lpad_size((int)std::max(P->vx.L, P->vy.L)));
}
int kernels_allow_view_tables(const fftup_plan* P)
{
    for (uint32_t L : {P->vx.L, P->vy.L}) {                   // (every L a view plan accepts passes: its two float2 buffers fit the LDS)
        if (L > (uint32_t)VT_MAX_L) return fail(FFTUP_E_UNSUPPORTED_SIZE, "k_view_tables: convolution length above " + std::to_string(VT_MAX_L));
        const StagePlan sp = make_stage_plan(L);
        for (int s = 0; s < sp.nstages; s++)
            if (!stage_fits_inplace((int)L, sp.radix[s], VT_THREADS, VT_PT)) return fail(FFTUP_E_UNSUPPORTED_SIZE, "k_view_tables: a stage does not fit its registers");
    }
    AllowLds allow;
    allow(view_tables_kernel(P));
    if (allow.err != hipSuccess) return fail(FFTUP_E_HIP, std::string("hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize): ") + hipGetErrorString(allow.err));
    return FFTUP_OK;
}
// shift: the frame's fftup_shift in device memory (fftup_execute_device_views_shifted; nullptr: none) -- k_view_tables moves the
// origins by its dx, dy when it runs; nothing the host derives here depends on the origin
static void frame_view(fftup_plan* P, int lane, const fftup_view& v, const fftup_shift* shift, Frame& f)
{
    fftup_plan::ViewTabs& t = P->vtabs[lane];
    struct Ax { const fftup_plan::ViewAxis* a; uint32_t N, M; double o, sp; ViewTables* out; };
    const Ax ax[2] = {{&P->vx, P->W, P->uW, v.origin_x, v.span_x, &f.vx}, {&P->vy, P->H, P->uH, v.origin_y, v.span_y, &f.vy}};
    ViewTabParams p{};
    for (int i = 0; i < 2; i++) {
        const Ax& x = ax[i];
        ViewTabAxis& q = p.ax[i];
        q.n = (int32_t)(P->mirror ? 2 * x.N : x.N); q.M = (int32_t)x.M; q.L = (int32_t)x.a->L;
        q.kmax = P->mirror ? fftup_viewtab::mirror_kmax_of(x.N, x.M, x.sp) : fftup_viewtab::kmax_of(x.N, x.M, x.sp);
        q.chirp = t.span[i] != x.sp;
        const fftup_viewphase::Pair o = fftup_viewphase::origin_of(x.o, (double)q.n, P->mirror);
        q.o_hi = o.hi; q.o_lo = o.lo; q.span = x.sp; q.plan = x.a->planL; q.tw = P->vroots[i];
        q.origin = x.o; q.mirror = P->mirror ? 1 : 0; q.shift = shift ? (i ? &shift->dy : &shift->dx) : nullptr;
        q.pre = t.pre[i]; q.post = t.post[i]; q.bhat = t.bhat[i];
        t.span[i] = x.sp; t.kmax[i] = q.kmax;
        *x.out = {q.kmax, q.pre, q.post, q.bhat};
    }
    t.built = true;
    f.ncols = P->mirror ? fftup_viewtab::mirror_ncols(P->W, f.vx.kmax) : f.vx.kmax + 1;
    f.NT = (f.ncols + P->TK - 1) / P->TK;
    const float u = view_factor(v, P->uW, P->uH);
    f.upsq = const_via_percent_f((double)(u * u), P->half);
    // (test builds, FFTUP_EXPERIMENT view_tables_time=1: the kernel alone between the plan's pair of timing events, reported on
    // stderr for tools/view_frames_time.py -- this waits for the lane, which the call otherwise never does)
    const char* ex = fftup_jit::experiment("view_tables_time");
    const bool timed = ex && atoi(ex) != 0;
    if (timed) (void)hipEventRecord(P->ev0, f.st);
    launch(view_tables_kernel(P), dim3(2), f.st, p);
    if (timed) {
        float ms = 0;
        (void)hipEventRecord(P->ev1, f.st);
        if (hipEventSynchronize(P->ev1) == hipSuccess && hipEventElapsedTime(&ms, P->ev0, P->ev1) == hipSuccess)
            fprintf(stderr, "fftup: k_view_tables %.3f us (chirp tables rebuilt: x %d, y %d)\n", (double)ms * 1e3, p.ax[0].chirp, p.ax[1].chirp);
    }
}

int launch_frame(fftup_plan* P, const FrameRun& r)
{
    Frame f = resolve(P, r);
    const bool tap = r.pass == Pass::presharpen_tap;
    if (f.kind == 0 && !tap) return fail(FFTUP_E_NO_INPUT, "no input uploaded for this slot");     // (the tap reads spectra only)
    if (r.view) {
        if (P->family != Family::view || (size_t)r.lane >= P->vtabs.size() || !P->vtabs[r.lane].pre[0]) return fail(FFTUP_E_INVALID_ARG, "a frame with a view of its own: not a view plan, or its lane has no tables");
        frame_view(P, r.lane, *r.view, r.shift, f);
    }
    const int rc = launch_family(P, f, r.pass);
    if (rc && r.view) P->vtabs[r.lane].span[0] = P->vtabs[r.lane].span[1] = 0;      // (a failed launch: the lane's chirp tables are nobody's)
    // what the frame left: its inverse rows have run, so the tap reads this lane's spectra, or its R unless the fused kernel ran instead
    if (tap || runs(r.pass, Pass::inverse)) { P->last_lane = r.lane; P->R_valid = !(P->fused && !tap); }
    return rc;
}

// ---- fftup_shift_path: one workgroup; the path of 4096 frames alone is 64 KB of LDS, so the kernel is allowed what this call needs
int launch_shift_path(const fftup_shift* in, fftup_shift* out, uint32_t n, uint32_t mode, float sigma, float min_peak, hipStream_t st)
{
    const Kern<ShiftPathParams> k = kern(k_shift_path, SP_THREADS, shift_path_lds((int)n, fftup_shiftpath::radius_of((double)sigma)));
    AllowLds allow;
    allow(k);
    if (allow.err != hipSuccess) return fail(FFTUP_E_HIP, std::string("hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize): ") + hipGetErrorString(allow.err));
    launch(k, dim3(1), st, ShiftPathParams{(const float*)in, (float*)out, (int32_t)n, mode, sigma, min_peak});
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FFTUP_E_HIP, std::string("fftup_shift_path: kernel launch: ") + hipGetErrorString(e));
    return FFTUP_OK;
}

// 64-bit wrapping sum of 32-bit words (fftup_output_checksum): per-thread partial sums, wave reduction, one atomic per wave
__global__ void __launch_bounds__(256) k_checksum(const uint32_t* __restrict__ w, size_t n, unsigned long long* sum)
{
    unsigned long long acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) acc += w[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(sum, acc);
}

void launch_checksum(fftup_plan* P, uint32_t slot, hipStream_t st)
{
    const size_t nbytes = (size_t)3 * P->uW * P->uH * (P->u8out ? 1 : P->esz), nwords = nbytes / 4;   // (uW, uH even: whole words for binary16 and bytes too)
    hipLaunchKernelGGL(k_checksum, dim3(1024), dim3(256), 0, st, (const uint32_t*)P->out[slot], nwords, (unsigned long long*)P->d_sum);
    // (FFTUP_FLAG_ODD_SIZE, binary16 planes with uW uH odd: two bytes are left over -- one more word, zero-extended)
    if (nbytes & 3)
        hipLaunchKernelGGL(k_checksum_tail, dim3(1), dim3(64), 0, st, (const uint8_t*)P->out[slot] + 4 * nwords, (int)(nbytes & 3), (unsigned long long*)P->d_sum);
}

#ifdef FFTUP_PLANE_STAMPS
// measurement build: the workgroups' begin / end stamps of the last frame's row and column pass (tools/plane_stamps.py)
extern "C" __attribute__((visibility("default"))) int fftup_debug_plane_stamps(unsigned long long* out)
{
    return out && hipMemcpyFromSymbol(out, HIP_SYMBOL(fftup::g_plane_stamps), sizeof(unsigned long long) * 3 * 2048 * 3) != hipSuccess;
}
#endif
