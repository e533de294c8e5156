// fftup_info.hip -- what the library reports behind the C ABI (include/fftup.h): a plan's description and byte counts
// (fftup_plan_describe, fftup_plan_info), error codes and the thread-local error text, the version, device enumeration.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "plan.hpp"

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
        char t[320];
        snprintf(t, sizeof t, "view%s: chirp-z resampling, rows %u->%u origin %.17g span %.17g (kmax %d, L=%u), columns %u->%u origin %.17g span %.17g (kmax %d, L=%u)",
                 P->mirror ? ", mirror (even reflection, period 2N)" : "", P->W, P->uW, P->vw.origin_x, P->vw.span_x, P->vx.kmax, P->vx.L, P->H, P->uH, P->vw.origin_y, P->vw.span_y, P->vy.kmax, P->vy.L);
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
        snprintf(info->kernel_names[0], 64, P->mirror ? "row_r2c_mirror" : "row_r2c_odd");
        snprintf(info->kernel_names[1], 64, P->mirror ? "col_view_mirror" : "col_view");
        snprintf(info->kernel_names[2], 64, P->mirror ? "row_view_c2r_mirror" : "row_view_c2r");
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
