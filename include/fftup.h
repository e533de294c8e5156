/*
 * fftup.h -- C ABI of the MI355X-native FFT upscaler (drop-in for VkResample's upscale path).
 *
 * The reference (DTolm/VkResample, one translation unit, no plugin layer) exposes the hot path as
 * the call sequence inside launchResample() (VkResample.cpp, "VR"); vkFFT/vkFFT.h is "VF".
 * Each entry point below replaces the reference calls cited next to it.  Plain pointers and
 * sizes only; no C++/torch types.  0 = success, non-zero = FFTUP_E_* (text: fftup_strerror).
 * The library never exits the process and never falls back to a CPU path: without a usable HIP
 * device every compute entry point fails with FFTUP_E_NO_DEVICE / FFTUP_E_HIP.
 *
 * Threading (mirrors VR:1282-1320, 1959-1969): one plan per host thread; a plan is used by one
 * thread at a time; distinct plans are independent (own stream, own device buffers).
 */
#ifndef FFTUP_H
#define FFTUP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define FFTUP_API __attribute__((visibility("default")))
#else
#define FFTUP_API
#endif

/* ---- error codes (reference: VkResult ints, 0 = VK_SUCCESS; VR:1286-1320, 1364-1367) ---- */
enum {
    FFTUP_OK = 0,
    FFTUP_E_INVALID_ARG = 1,    /* null pointer, bad slot, odd size (without FFTUP_FLAG_ODD_SIZE), channels != 3 (VR:1368) */
    FFTUP_E_UNSUPPORTED_SIZE = 2, /* a dimension is not 2,3,5,7-smooth: VF:4719-4726
                                     (VK_ERROR_FORMAT_NOT_SUPPORTED); with FFTUP_FLAG_ANY_SIZE: such a
                                     dimension is longer than 4096, or the plan is outside that flag's
                                     bounds (fftup_last_error says which)                              */
    FFTUP_E_UNSUPPORTED_PRECISION = 3, /* -p must be 0, 1 or 2                                         */
    FFTUP_E_NO_DEVICE = 4,      /* no HIP device / bad device id (VR:1292-1296)                         */
    FFTUP_E_HIP = 5,            /* a HIP runtime call failed (message in fftup_last_error)              */
    FFTUP_E_OUT_OF_MEMORY = 6,  /* device allocation failed (allocateFFTBuffer VR:361-384)              */
    FFTUP_E_NO_INPUT = 7,       /* execute/download before any upload                                   */
    FFTUP_E_INCOMPLETE = 8,     /* "Image not found" class of errors in the host mirror (VR:1366)       */
    FFTUP_E_WOULD_BLOCK = 9,    /* fftup_submit_png / fftup_submit_rgb8: every ring slot holds an uncollected PNG ticket of the
                                   CALLING thread and no other thread has collected anything on this plan (after a bounded
                                   wait, FFTUP_SELF_WAIT_MS, default 2000) -- waiting would never end            */
    FFTUP_E_OVERFLOW = 10       /* fftup_wait_png: the frame's deflate stream did not fit the encoder's buffer; nothing was
                                   written beyond it, the frame is not encoded                                   */
};

/* ---- flags ---- */
enum {
    FFTUP_FLAG_U8_WRAP = 1u,       /* u8 store wraps like the x86 C cast of VR:1715 instead of saturating */
    FFTUP_FLAG_FUSE_U8_LOAD = 2u,  /* row-FFT kernel reads the uint8 RGB image directly (README.md:31
                                      roadmap item); otherwise upload converts to the reference's planar
                                      float/half inputBuffer first (VR:1636-1688 semantics)               */
    FFTUP_FLAG_GENERIC_KERNELS = 4u, /* force the size-generic kernels even where a tuned plan exists    */
    FFTUP_FLAG_UNFUSED_SHARPEN = 8u, /* keep C2R and sharpen as two launches with the pre-sharpen image in
                                        HBM, like the reference (tempBuffer); default fuses them          */
    FFTUP_FLAG_TUNE_PLAN = 16u,      /* plans specialised at plan time (below): compile and time the alternatives for the fused
                                        kernel's factorization on the device, keep the fastest, remember it in
                                        <cache dir>/wisdom.txt (a few seconds, once per row length and device)            */
    FFTUP_FLAG_FUSE_U8_STORE = 32u,  /* 8-bit pipelines (the reference's own: PNG in, PNG out): the fused C2R+sharpen kernel stores
                                        the interleaved 8-bit RGB image itself (the conversion of VR:1708-1748 in registers); the
                                        float / half planes are never written, fftup_download_rgb8 / fftup_submit_rgb8 need no
                                        conversion launch, fftup_download_planar fails with FFTUP_E_INVALID_ARG.  Plans without a
                                        fused kernel (size-generic, -p 1, non-R2C, FFTUP_FLAG_UNFUSED_SHARPEN) ignore the flag:
                                        fftup_info.u8_store says which it is                                               */
    FFTUP_FLAG_SEQUENTIAL_EXECUTE = 64u, /* accepted and ignored: ordered iterations are what fftup_execute does (0.6 and earlier
                                        needed this flag for it)                                                               */
    FFTUP_FLAG_OVERLAP_ITERATIONS = 128u, /* EXTENSION, not the reference's semantics: the n_iter identical iterations of one
                                        fftup_execute call alternate on the plan's streams and overlap like the distinct frames
                                        of fftup_execute_ring (a throughput figure; same bits).  A plan without a ring is then
                                        laid out for overlapping frames (one strip of the last kernel per compute unit)         */
    FFTUP_FLAG_DCT = 256u,           /* EXTENSION (0.7.0; older libraries ignore the bit): DCT upscale instead of the FFT's -- the
                                        image is not treated as periodic, so a frame whose opposite borders differ gets no ringing
                                        there.  Per axis, separable, input x[n] (n < N), output y[m] (m < M = (uint32_t)(u N), the
                                        FFT path's size rule):  X[k] = sum_n x[n] cos(pi k (2n+1) / 2N)  (DCT-II), then
                                        y[m] = X[0]/N + (2/N) sum_{k=1}^{N-1} X[k] cos(pi k (2m+1) / 2M)  (DCT-III of the
                                        zero-padded coefficients).  Samples sit at pixel CENTRES: output pixel m lies at input
                                        position (m + 1/2) N / M - 1/2, where the FFT path puts pixel 0 on pixel 0.  Constants
                                        stay constant, -u 1 reproduces the input, no Nyquist special case (the FFT path's quirks
                                        B1 / B2 do not apply).  The pre-sharpen image R keeps the FFT path's convention upsq R = y
                                        and the sharpen pass is the FFT path's, unchanged (its wrap at the right edge, quirk B5,
                                        included).  Four launches, size-generic kernels: the plan-time, ahead-of-time and fused
                                        kernels and FFTUP_FLAG_FUSE_U8_STORE do not apply (fftup_info.tuned = u8_store = 0).
                                        Accepted: -p 0 and -p 2 (-p 1: FFTUP_E_UNSUPPORTED_PRECISION), u*W <= 8192 and columns
                                        whose transforms fit the compute unit's local memory (no four-step DCT):
                                        FFTUP_E_UNSUPPORTED_SIZE otherwise                                                     */
    FFTUP_FLAG_DOWNSCALE = 512u,     /* EXTENSION: spectral DOWNSCALE, upscale in [0.125, 1) (FFTUP_E_INVALID_ARG otherwise; without
                                        the flag a factor below 1 stays FFTUP_E_INVALID_ARG, so a library without this mode refuses
                                        such a plan).  Output sizes by the usual rule uW = (uint32_t)(u W), uH = (uint32_t)(u H) in
                                        fp32: even, at least 2 and below W, H (FFTUP_E_INVALID_ARG), 2,3,5,7-smooth
                                        (FFTUP_E_UNSUPPORTED_SIZE).  FFT mode: per axis, separable, input x[n] (n < N), output length
                                        M < N, h = M/2, X = DFT(x) unnormalised; the spectrum is cropped with its Nyquist bins folded,
                                          Y[k] = X[k] (k < h),  Y[h] = X[h] + X[N-h],  Y[M-k] = X[N-k] (0 < k < h),
                                        and R = (1/M) IDFT_M(Y) per axis; the amplitude-preserving image is y = R (uW uH) / (W H).
                                        Per axis this is scipy.signal.resample: ideal band-limited decimation, output pixel m on
                                        input position m N / M (pixel 0 on pixel 0, as the upscale path), constants stay constant,
                                        content above the new Nyquist frequency vanishes (quirks B1-B3 do not apply).  The sharpen
                                        pass is the upscale path's, unchanged (upsq = "%f"(u u), quirk B5).
                                        With FFTUP_FLAG_DCT: the DCT mode's formula with the coefficients truncated instead of
                                        zero-padded, y[m] = X[0]/N + (2/N) sum_{k=1}^{M-1} X[k] cos(pi k (2m+1) / 2M), R = y / upsq.
                                        Four launches, size-generic kernels (fftup_info.tuned = u8_store = 0; FFTUP_FLAG_FUSE_U8_STORE,
                                        _GENERIC_KERNELS, _UNFUSED_SHARPEN and _TUNE_PLAN are accepted and change nothing).
                                        Accepted: -p 0 and -p 2 (-p 1: FFTUP_E_UNSUPPORTED_PRECISION), W <= 8192 and columns whose
                                        transforms fit the compute unit's local memory: FFTUP_E_UNSUPPORTED_SIZE otherwise       */
    FFTUP_FLAG_ANY_SIZE = 1024u,     /* EXTENSION: widens the set of accepted SIZES and changes nothing else.  Without the flag: the
                                        reference's rule, every length (W, H, uW, uH) 2,3,5,7-smooth.  With it, on a plan whose four
                                        lengths are smooth: a no-op -- same kernels (ahead-of-time and plan-time ones included), same
                                        fftup_info, same output bytes.  Otherwise: the lengths still have to be even and at least 2
                                        (uW = (uint32_t)(u W), uH = (uint32_t)(u H); odd: FFTUP_E_INVALID_ARG), and a length with a
                                        prime factor above 7 is accepted if it is at most 4096 (beyond: FFTUP_E_UNSUPPORTED_SIZE).
                                        Such a transform runs as a chirp-z (Bluestein) transform through a smooth length
                                        L >= 2N - 1 (L <= 8192); the smooth lengths of the same plan keep their Stockham transforms.
                                        The result is the reference's filter at that size, per axis and separable: forward DFT, the
                                        centred zero-pad with quirks B1-B3, inverse DFT, then the sharpen pass unchanged (B4, B5,
                                        upsq = "%f"(u u)).  With FFTUP_FLAG_DOWNSCALE (FFT mode): that flag's formula, W <= 8192.
                                        A plan with a non-smooth length runs the size-generic R2C kernels (fftup_info.tuned =
                                        u8_store = 0, kernel names with a "_bz" suffix where a Bluestein transform runs;
                                        FFTUP_FLAG_FUSE_U8_STORE, _GENERIC_KERNELS, _UNFUSED_SHARPEN and _TUNE_PLAN are accepted and
                                        change nothing; FFTUP_FLAG_FUSE_U8_LOAD and every execution path work as on other plans), and
                                        is accepted for -p 0 and -p 2 (-p 1: FFTUP_E_UNSUPPORTED_PRECISION), rows of at most 8192
                                        points and columns whose transforms fit the compute unit's local memory (no non-R2C or
                                        four-step path beside a Bluestein transform: FFTUP_E_UNSUPPORTED_SIZE).  With FFTUP_FLAG_DCT
                                        a non-smooth length stays FFTUP_E_UNSUPPORTED_SIZE (the DCT kernels' 2N / 4N packing is not
                                        covered), with or without FFTUP_FLAG_DOWNSCALE.  All of this is arithmetic on the sizes,
                                        decided before any device access.  fftup_jit_check keeps returning FFTUP_E_UNSUPPORTED_SIZE
                                        for these sizes, and fftup_version() is unchanged: detect the mode by creating a plan -- a
                                        library without it returns FFTUP_E_UNSUPPORTED_SIZE for 46x22 with the flag set         */
    FFTUP_FLAG_ODD_SIZE = 2048u,     /* EXTENSION: accepts odd widths and heights, input or output, and changes nothing else.
                                        Without the flag: an odd W, H, uW or uH is FFTUP_E_INVALID_ARG, as before (also with
                                        FFTUP_FLAG_ANY_SIZE alone).  With it, on a plan whose four lengths are even: a no-op -- same
                                        kernels (ahead-of-time and plan-time ones included), same fftup_info, same output bytes.
                                        With it and at least one of W, H, uW, uH odd: sizes follow the usual rule
                                        uW = (uint32_t)(u W), uH = (uint32_t)(u H) in fp32, each length at least 2, and the plan
                                        computes EXACT TRIGONOMETRIC RESAMPLING per axis, separably (scipy.signal.resample's rule,
                                        the one FFTUP_FLAG_DOWNSCALE names).  Per axis, input x[n], n < N, output length M,
                                        X = DFT_N(x), K = min(N, M): the bins |k| < K/2 are copied, Y[k mod M] = X[k mod N]; if K
                                        is even its Nyquist bin h = K/2 is split for M > N, Y[h] = Y[M-h] = X[h]/2, folded for
                                        M < N, Y[h] = X[h] + X[N-h] (FFTUP_FLAG_DOWNSCALE's rule, unchanged), kept for M = N; every
                                        other bin of Y is 0.  The pre-sharpen image is R = 1/(uW uH) IDFT(Y) over both axes, the
                                        amplitude-preserving image y = R (uW uH) / (W H): constants stay constant, -u 1 reproduces
                                        the input, output pixel m sits at input position m N / M.  The quirks B1-B3 of the
                                        reference's even-size path do NOT apply on either axis of such a plan (an even axis beside
                                        an odd one included).  The sharpen pass is the existing one, unchanged (upsq = "%f"(u u),
                                        quirks B4 and B5).  A 2,3,5,7-smooth odd length runs the Stockham stages; a length with a
                                        prime factor above 7, odd or even, needs FFTUP_FLAG_ANY_SIZE as well, must be at most 4096
                                        and runs as a Bluestein transform (without that flag, or above 4096:
                                        FFTUP_E_UNSUPPORTED_SIZE).  With FFTUP_FLAG_DOWNSCALE (FFT mode): factors in [0.125, 1),
                                        output lengths below the input's.  Bounds as for Bluestein plans: -p 0 and -p 2 (-p 1:
                                        FFTUP_E_UNSUPPORTED_PRECISION), rows of at most 8192 points, columns whose transforms fit
                                        the compute unit's local memory (no non-R2C or four-step path: FFTUP_E_UNSUPPORTED_SIZE);
                                        with FFTUP_FLAG_DCT an odd length is FFTUP_E_UNSUPPORTED_SIZE.  Such a plan runs four
                                        launches of size-generic kernels (fftup_info.tuned = u8_store = 0, the three transform
                                        kernels' names carry "_odd", and "_bz" behind it where a Bluestein transform runs);
                                        FFTUP_FLAG_FUSE_U8_STORE, _GENERIC_KERNELS, _UNFUSED_SHARPEN and _TUNE_PLAN are accepted and
                                        change nothing; FFTUP_FLAG_FUSE_U8_LOAD and every execution path work as on other plans.
                                        fftup_output_checksum of binary16 planes with uW uH odd: the two bytes behind the last
                                        whole word enter the sum as one more word, zero-extended.  All of this is arithmetic on the
                                        sizes, decided before any device access.  fftup_jit_check keeps returning
                                        FFTUP_E_UNSUPPORTED_SIZE for these sizes, and fftup_version() is unchanged: detect the mode
                                        by creating a plan -- a library without it returns FFTUP_E_INVALID_ARG for 45x21 -u 2 with
                                        the flag set                                                                            */
    FFTUP_FLAG_MIRROR = 4096u        /* EXTENSION: a view plan (fftup_plan_create_view, below) WITHOUT the wrap-around border.  Valid
                                        on fftup_plan_create_view only; fftup_plan_set_view keeps working on such a plan.  Per axis,
                                        separable.  The input is x[n], n < N.  The output has M points.  The view is (origin, span)
                                        with step s = span / M.  Output pixel m sits at t_m = origin + m s.
                                        With FFTUP_FLAG_MIRROR the frame is continued by its half-sample even reflection:
                                        x~[n] = x[n] for n < N, x~[n] = x[2N-1-n] for N <= n < 2N, with period 2N.  The plan
                                        evaluates the view formula of that extended frame.  In closed form:
                                          C[k]  = sum_n x[n] cos(pi k (2n+1) / 2N)                         (DCT-II, k = 0 .. N-1)
                                          kmax  = min(N - 1, floor((double)(N M) / max(span, (double)M)))
                                          y[m]  = C[0]/N + (2/N) sum_{k=1..kmax} C[k] cos(pi k (2 t_m + 1) / 2N)
                                        This equals the view formula below at period 2N applied to x~.  Bin N of the extension is
                                        identically zero, so capping kmax at N-1 changes nothing.  Constants stay constant; a view
                                        that touches a border mixes in the frame's own reflection instead of the opposite border,
                                        and a view with origin < 0 or span > N shows reflected copies of the frame instead of
                                        wrapped ones.  With origin = (N/M - 1)/2 and span = N it is FFTUP_FLAG_DCT's map (that
                                        flag's upscale formula for M >= N, its downscale formula for M < N).
                                        The pre-sharpen image is R = y span_x span_y / (uW uH).  The effective factor is u_e, as
                                        for every view plan.  The sharpen pass is the view plans' own, unchanged, with quirks B4
                                        and B5.
                                        Rules, all arithmetic on the sizes and decided before any device access:
                                        fftup_plan_create and fftup_plan_create_size return FFTUP_E_INVALID_ARG with the flag set;
                                        with FFTUP_FLAG_DCT the view plans' FFTUP_E_UNSUPPORTED_SIZE stays; -p 1 is
                                        FFTUP_E_UNSUPPORTED_PRECISION; width <= 8192; the step stays in [1/64, 8];
                                        FFTUP_FLAG_ANY_SIZE keeps its meaning for width and height (the forward transforms stay
                                        at lengths W and H -- the DCT-II of N points runs as ONE transform of N points -- Bluestein
                                        where non-smooth, <= 4096).  The convolution lengths are those of the doubled period: the
                                        smallest 2,3,5,7-smooth L >= 2N + M per axis.  Rows need L_x <= 8192 (1920 -> 3840: 7680,
                                        2048 -> 4096: 8192), columns two local-memory buffers of max(H or its Bluestein length,
                                        L_y) points at a tile width of 1: FFTUP_E_UNSUPPORTED_SIZE otherwise.
                                        Four launches (fftup_info.tuned = u8_store = 0; kernel names row_r2c_mirror[_bz],
                                        col_view_mirror[_bz], row_view_c2r_mirror, sharpen; fftup_plan_describe says "mirror");
                                        every execution path works on such a plan unchanged.  A library without the mode ignores
                                        the bit and returns the periodic view: detect the mode by kernel names carrying "_mirror",
                                        fftup_version() is unchanged                                                             */
};

/* Replaces VkResampleConfiguration (VR:45-59) + the part of VkFFTConfiguration (VF:22-94) that
 * launchResample() derives from it (VR:1409-1503). */
typedef struct fftup_config {
    uint32_t width, height;   /* input image size; both even (odd: FFTUP_FLAG_ODD_SIZE)                */
    uint32_t channels;        /* must be 3 (stbi_load(...,3) VR:1362, channels = 3 VR:1368)           */
    float    upscale;         /* -u; output = (uint32_t)(upscale*size) (VR:1417-1418)                */
    uint32_t precision;       /* -p: 0 single, 1 double (VR:1422), 2 half-memory/fp32-math (VR:1420-1421) */
    float    sharpen;         /* -s sharpening constant (VR:1616)                                    */
    int32_t  device;          /* -d HIP device ordinal                                               */
    uint32_t flags;           /* FFTUP_FLAG_*                                                        */
    uint32_t ring;            /* resident input/output frame slots (0 or 1 = one, like the reference; <= 1024) */
} fftup_config;

/* Environment read by fftup_plan_create (operational knobs, not part of the reference's surface):
 *   FFTUP_STREAMS=n     HIP streams consecutive frames of fftup_execute_ring / fftup_submit_rgb8 (and the iterations of
 *                       fftup_execute under FFTUP_FLAG_OVERLAP_ITERATIONS) alternate on (default 3, 1..4)
 *   FFTUP_JIT=0|1       run-time specialised plans (default 1); FFTUP_JIT_VERBOSE=1 prints why one fell back
 *   FFTUP_CACHE_DIR     code-object cache and wisdom file of those plans (default ~/.cache/fftup);
 *   FFTUP_KERNEL_DIR    kernel headers, when not the ones embedded in the library; FFTUP_HIPRTC_LIB: the run-time compiler's
 *                       shared object (default: libhiprtc.so of the ROCm install) */

typedef struct fftup_plan fftup_plan;   /* opaque; replaces VkGPU + 2x VkFFTApplication +
                                           2x VkShiftApplication + the three device buffers      */

enum { FFTUP_NUM_KERNELS = 4 };          /* row R2C, column fwd+pad+inv, row C2R, sharpen        */

/* ABI: fields are only ever APPENDED to this struct; `abi_version` (== FFTUP_ABI_VERSION of the library that filled it) says
 * how far it is valid: 1 = up to kernel_names, 2 = + kernel_min_bytes, tuned may be 2, abi_version itself.
 * (0.2.x builds had kernel_min_bytes in front of device_bytes: callers built against those must be rebuilt.) */
enum { FFTUP_ABI_VERSION = 2 };
typedef struct fftup_info {
    uint32_t out_width, out_height;      /* uW, uH                                                */
    uint32_t num_kernels;                /* launches per frame                                    */
    uint32_t tuned;                      /* 0: size-generic kernels, non-zero: size-specialised (1: ahead-of-time, 2: at plan time through hipRTC) */
    double   alg_bytes_per_frame;        /* B_alg of SURVEY 8(d) for this plan's I/O types        */
    double   kernel_alg_bytes[FFTUP_NUM_KERNELS]; /* algorithmic bytes of each kernel: a fused C2R+sharpen
                                                     launch keeps S2 + 2R + out although R never reaches HBM          */
    uint64_t device_bytes;               /* device memory owned by the plan ("VRAM per thread")   */
    char     device_name[256];
    char     kernel_names[FFTUP_NUM_KERNELS][64];
    /* ---- appended in ABI version 2 ---- */
    double   kernel_min_bytes[FFTUP_NUM_KERNELS]; /* bytes each kernel has to move through HBM as implemented
                                                     (e.g. fused: spectrum rows incl. strip halos + out)               */
    uint32_t abi_version;                /* FFTUP_ABI_VERSION of the library                      */
    uint32_t u8_store;                   /* 1: the plan's output slots hold 8-bit RGB (FFTUP_FLAG_FUSE_U8_STORE in effect)     */
} fftup_info;

/* devices_list() VR:239-268 */
FFTUP_API int fftup_device_count(void);
FFTUP_API int fftup_device_name(int device, char* buf, size_t buflen);
/* PCI bus id ("0000:c1:00.0") of a device: job accounting of multi-GPU runs (one process / thread per GPU: the ids of a
 * job's ranks must all differ) */
FFTUP_API int fftup_device_pci_bus_id(int device, char* buf, size_t buflen);

/* initializeVulkanFFT x2 + createShiftApp + createSharpenApp + 3x allocateFFTBuffer
 * (VR:1437-1448, 1506-1509, 1562, 1617).  Every even 2,3,5,7-smooth width and height up to 65536 whose upscaled sizes are
 * even and smooth is a valid plan, as in the reference: upscaled widths beyond 8192 (4096 for -p 1) take the reference's
 * non-R2C path (VR:1424); rows and columns too long for the compute unit's local memory run as two-launch "four-step"
 * transforms through device memory (the reference's multi-upload plans, VF:4773-4992).  fftup_plan_describe says which.
 * FFTUP_FLAG_DCT plans accept a subset of these sizes (see the flag); FFTUP_FLAG_DOWNSCALE plans take factors below 1;
 * FFTUP_FLAG_ANY_SIZE lifts the smoothness rule for even lengths up to 4096 (Bluestein transforms, see the flag);
 * FFTUP_FLAG_ODD_SIZE accepts odd lengths (exact trigonometric resampling, see the flag). */
FFTUP_API int fftup_plan_create(fftup_plan** out, const fftup_config* cfg);
/* EXTENSION: a plan for an exact output size, one factor per axis ("make this frame out_width x out_height": 1366x768 -> 1920x1080,
 * anamorphic 720x576 -> 1920x1080, one axis only, one axis up and the other down).  cfg->upscale is ignored; every other field means
 * what it means for fftup_plan_create, and the plan is an ordinary plan: every upload, execute, ring, submit, PNG, download,
 * checksum, info and describe entry point works on it unchanged.
 * Such a plan ALWAYS computes the exact trigonometric resampling written at FFTUP_FLAG_ODD_SIZE, on both axes, whatever the
 * parities and whatever the direction of each axis (up on one, down or equal on the other); the quirks B1-B3 never apply.
 * FFTUP_FLAG_ODD_SIZE and FFTUP_FLAG_DOWNSCALE are implied (accepted, they change nothing); FFTUP_FLAG_ANY_SIZE keeps its meaning
 * (a length with a prime factor above 7 needs it and must be at most 4096: FFTUP_E_UNSUPPORTED_SIZE otherwise).
 * align = FFTUP_ALIGN_CORNER: output pixel 0 on input pixel 0 (pixel m at input position m N / M), as every other FFT plan.
 * align = FFTUP_ALIGN_CENTRE: pixel centres aligned, as OpenCV, PIL and FFTUP_FLAG_DCT place them: per axis N -> M, with
 * d = (N/M - 1)/2, the bin of signed frequency f carries the extra factor exp(+2 pi i f d / N) (DFT with exp(-2 pi i nk / N)):
 *   copied bins   Y[f mod M] = X[f mod N] exp(2 pi i f d / N);
 *   split Nyquist bin (M > N, N even, h = N/2):    Y[h] = X[h] exp(+i phi) / 2,  Y[M-h] = X[h] exp(-i phi) / 2,  phi = 2 pi h d / N;
 *   folded Nyquist bin (M < N, M even, h = M/2):   Y[h] = X[h] exp(+i phi) + X[N-h] exp(-i phi)  (real);
 *   M = N: d = 0, nothing changes.
 * Output pixel m then sits at input position (m + 1/2) N / M - 1/2: constants stay constant, a cosine of k cycles comes back as the
 * same cosine sampled at those positions, and mirroring the input mirrors the output (under FFTUP_ALIGN_CORNER it does not).
 * The pre-sharpen image is R = 1/(uW uH) IDFT(Y), the amplitude-preserving image y = R (uW uH) / (W H).  The sharpen pass is the
 * existing one, unchanged (quirks B4, B5), with the effective factor u_e = (float)sqrt((double)uW uH / ((double)W H)) in the place
 * of cfg->upscale: upsq = "%f"(u_e u_e), the product formed in fp32.
 * Bounds (arithmetic on the sizes, decided before any device access; fftup_last_error names the rule): FFTUP_E_INVALID_ARG for a
 * length below 2, align above 1, an output length outside [N/8, 8 N] on either axis, channels != 3, null pointers;
 * FFTUP_E_UNSUPPORTED_PRECISION for -p 1; FFTUP_E_UNSUPPORTED_SIZE with FFTUP_FLAG_DCT, for rows above 8192 points and for columns
 * whose transforms do not fit the compute unit's local memory (the odd-size plans' limits).  Four launches of the odd-size plans'
 * kernels (fftup_info.tuned = u8_store = 0, names with "_odd", "_crop" on an axis that shrinks, "_bz" where a Bluestein transform
 * runs).  fftup_version() is unchanged: detect the mode by this symbol. */
enum { FFTUP_ALIGN_CORNER = 0, FFTUP_ALIGN_CENTRE = 1 };
FFTUP_API int fftup_plan_create_size(fftup_plan** out, const fftup_config* cfg,
                                     uint32_t out_width, uint32_t out_height, uint32_t align);
/* EXTENSION: a VIEW plan -- zoom into a region, pan by a fraction of a pixel, scale by any real ratio.  The out_width x out_height
 * output shows the rectangle of the frame that starts at input position (origin_x, origin_y) and is (span_x, span_y) input pixels
 * wide and high: per axis N -> M with step s = span / M, output pixel m sits at input position t_m = origin + m s (pixel indices as
 * coordinates, the frame periodic with period N).  The plan evaluates the frame's trigonometric interpolant there, separably:
 * with X[f] = sum_n x[n] exp(-2 pi i nf / N),
 *   kmax = min(N/2 (integer division), floor((double)(N M) / (2 max(span, (double)M)))),   g_f = 1/2 if 2 |f| == N, else 1,
 *   y[m] = (1/N) sum_{f = -kmax .. kmax} g_f X[f mod N] exp(2 pi i f t_m / N).
 * For s <= 1 this is the full interpolant (an even N's Nyquist bin enters as X[N/2] cos(pi t)); for s > 1 the spectrum is truncated
 * at the output's Nyquist frequency: no aliasing.  It interpolates the WHOLE frame, so an interior view has no seam (cropping first
 * would make the crop periodic).  origin = 0, span = N is fftup_plan_create_size with FFTUP_ALIGN_CORNER, origin = (N/M - 1)/2 with
 * FFTUP_ALIGN_CENTRE (the fold, split and kept rules of FFTUP_FLAG_ODD_SIZE follow from kmax and g).  A rectangle given in
 * pixel-EDGE coordinates [x0, x0 + w) with the centres aligned is origin = x0 + w/(2M) - 1/2, span = w.
 * The pre-sharpen image is R = y span_x span_y / (uW uH); the sharpen pass is the existing one, unchanged (quirks B4, B5), with the
 * effective factor u_e = (float)sqrt((double)uW uH / (span_x span_y)) in the place of cfg->upscale: upsq = "%f"(u_e u_e), the product
 * formed in fp32.
 * cfg->upscale is ignored; every other field means what it means for fftup_plan_create_size, and the plan is an ordinary plan: upload,
 * execute, ring, submit, PNG, download, checksum, fftup_execute_device, info and describe work on it unchanged.  FFTUP_FLAG_ODD_SIZE and
 * FFTUP_FLAG_DOWNSCALE are implied; FFTUP_FLAG_ANY_SIZE keeps its meaning and matters for width and height only (the forward
 * transforms are the only ones of the input's lengths; out_width and out_height may be any numbers).
 * Each axis runs as a chirp-z transform: a cyclic convolution of a 2,3,5,7-smooth length L >= 2 (N/2) + M, fixed by N and M.  Four
 * launches (fftup_info.tuned = u8_store = 0; kernel names row_r2c_odd[_bz], col_view[_bz], row_view_c2r, sharpen).
 * Bounds (arithmetic, decided before any device access; fftup_last_error names the rule): FFTUP_E_INVALID_ARG for null pointers,
 * channels != 3, a length below 2, a non-finite origin or span, a step span / M outside [1/64, 8] on either axis;
 * FFTUP_E_UNSUPPORTED_PRECISION for -p 1; FFTUP_E_UNSUPPORTED_SIZE with FFTUP_FLAG_DCT, for width > 8192, for a row convolution length
 * above 8192, for a width or height with a prime factor above 7 without FFTUP_FLAG_ANY_SIZE or above 4096, and for columns whose two
 * local-memory buffers do not fit at a tile width of 1.  fftup_version() is unchanged: detect the mode by this symbol.
 *
 * fftup_plan_set_view re-aims a view plan without re-creating it (a pan or a zoom per frame): it waits for the plan's own streams,
 * rebuilds the host tables and uploads them -- blocking; frames executed afterwards show the new view.  Everything is sized for the
 * worst case of the plan's four lengths at creation, so every valid view fits.  FFTUP_E_INVALID_ARG: a null pointer, a plan that is
 * not a view plan, a non-finite value, a step outside [1/64, 8]; the plan then keeps its view. */
typedef struct fftup_view { double origin_x, origin_y, span_x, span_y; } fftup_view;
FFTUP_API int fftup_plan_create_view(fftup_plan** out, const fftup_config* cfg,
                                     uint32_t out_width, uint32_t out_height, const fftup_view* view);
FFTUP_API int fftup_plan_set_view(fftup_plan* plan, const fftup_view* view);
/* deleteVulkanFFT x2, deleteShiftApp x2, buffer frees (VR:1759-1771) */
FFTUP_API void fftup_plan_destroy(fftup_plan* plan);
FFTUP_API int fftup_plan_info(const fftup_plan* plan, fftup_info* info);
/* one line saying which kernels the plan runs (for a plan specialised at plan time: the chosen factorizations) */
FFTUP_API int fftup_plan_describe(const fftup_plan* plan, char* buf, size_t buflen);

/* Run-time specialised plans (csrc/jit.hpp; the counterpart of VkFFT generating and compiling its shaders for the
 * requested size at plan time, VF:4707-5189 + the GLSL generator, glslang in VkResample's link line).  A plan with an
 * integer, half-, quarter- or eighth-integer upscale factor or a ratio over 3, 5 or 7 whose sizes come out exact (-u 1.125, 1.2, 1.25, 4/3, 1.4, 1.5, 1.6, 5/3, 1.75, 1.875, 2, 2.25, 2.5, 8/3, 3, 3.5, 4, 5, 6, 7, 8; -p 0 / -p 2; H <= 8192,
 * u*W <= 8192, 4 | u*W, u*H even)
 * whose size has no ahead-of-time
 * kernels gets its row, column and fused C2R+sharpen kernels
 * instantiated for exactly that size through hipRTC inside fftup_plan_create; fftup_info.tuned is then 2.  FFTUP_JIT=0
 * or FFTUP_FLAG_GENERIC_KERNELS keeps such plans on the size-generic kernels (as does a missing libhiprtc.so).
 * fftup_jit_check does the same WITHOUT a device: picks the factorizations, compiles for `arch` (NULL: gfx950; "": does not
 * compile) and writes a one-line description.  FFTUP_E_UNSUPPORTED_SIZE: no specialised factorization (the generic kernels run that
 * size); FFTUP_E_HIP: hipRTC unavailable or compilation failed (fftup_last_error has the log). */
FFTUP_API int fftup_jit_check(uint32_t width, uint32_t height, float upscale, uint32_t precision, const char* arch,
                              char* desc, size_t desclen);

/* host pack loop + transferDataFromCPU (VR:1636-1688).  rgb: interleaved 8-bit RGB, H rows of
 * row_stride_bytes (>= 3*W).  Blocking, like the reference. */
FFTUP_API int fftup_upload_rgb8(fftup_plan* plan, const uint8_t* rgb, size_t row_stride_bytes);
FFTUP_API int fftup_upload_rgb8_slot(fftup_plan* plan, uint32_t slot, const uint8_t* rgb, size_t row_stride_bytes);
/* transferDataFromCPU of an already packed planar buffer: float (precision 0), double (precision 1) or IEEE
 * half (precision 2) planes, 3 planes of H rows; strides in elements (the reference's inputBuffer uses
 * row stride W and plane stride (W+2)*H, VR:1644). */
FFTUP_API int fftup_upload_planar(fftup_plan* plan, uint32_t slot, const void* planes,
                                  size_t row_stride_elems, size_t plane_stride_elems);

/* performVulkanUpscale (VR:1249-1279): enqueue n_iter full pipelines, one synchronisation.
 * *ms_per_iter = device time from before the first to after the last launch, divided by n_iter -- the
 * reference's "Time: X ms" (VR:1270-1278).  Every iteration reads input slot 0 and computes the same frame; output slot 0
 * holds it afterwards.  The reference records the n_iter pipelines into ONE command buffer on ONE queue, and every stage ends
 * in a compute-to-compute pipeline barrier (vkFFT.h:7678, VR:1217): iteration i + 1 cannot start before the sharpen pass of
 * iteration i has finished.  So here: one stream, the iterations in order, nothing overlaps -- single-frame latency, the figure
 * that is comparable with the reference's.  FFTUP_FLAG_OVERLAP_ITERATIONS (an extension) lets the identical iterations of a
 * call alternate on the plan's FFTUP_STREAMS streams instead (own spectra, own scratch output per stream beyond the first,
 * allocated on the first such call): the same bits, the throughput figure of fftup_execute_ring. */
FFTUP_API int fftup_execute(fftup_plan* plan, uint32_t n_iter, double* ms_per_iter);
/* batched mode: n_frames pipelines, frame i reads input slot (first_slot+i) % ring and writes
 * output slot (first_slot+i) % ring; returns total device milliseconds. */
FFTUP_API int fftup_execute_ring(fftup_plan* plan, uint32_t n_frames, uint32_t first_slot, double* ms_total);
/* the same batch with a HIP event before and after every kernel launch of every `stride`-th frame, recorded on
 * the stream that runs the kernel: also returns the average duration (ms) of each of the plan's kernels.  Consecutive
 * frames run on two streams, so a kernel's duration includes the time it shares the GPU with the other
 * stream's kernels (fftup_profile_kernels gives the isolated durations). */
FFTUP_API int fftup_execute_ring_timed(fftup_plan* plan, uint32_t n_frames, uint32_t first_slot, uint32_t stride,
                                       double* ms_total, double* ms_per_kernel);
/* measurement aid: runs n_iter frames with a HIP event pair around every kernel launch on the
 * plan's stream and returns the average duration (ms) of each of the FFTUP_NUM_KERNELS kernels, net of the
 * duration of an empty event pair measured in the same loop (unused slots read 0). */
FFTUP_API int fftup_profile_kernels(fftup_plan* plan, uint32_t n_iter, double* ms_per_kernel);

/* transferDataToCPU + unpack loop (VR:1697-1748).  rgb8: u8 = trunc(255*x), saturating unless
 * FFTUP_FLAG_U8_WRAP.  planar: dense [3][uH][uW] float (precision 0), double (1) or half (2). */
FFTUP_API int fftup_download_rgb8(fftup_plan* plan, uint32_t slot, uint8_t* rgb, size_t row_stride_bytes);
FFTUP_API int fftup_download_planar(fftup_plan* plan, uint32_t slot, void* planes);
/* parity-test taps: the C2R output before sharpening (the reference's tempBuffer contents,
 * dense [3][uH][uW]) of the last executed frame -- on the non-R2C path (uW > 8192, VR:1424) the real
 * part of the complex image -- and the converted input planes [3][H][W]. */
FFTUP_API int fftup_download_presharpen(fftup_plan* plan, void* planes);
FFTUP_API int fftup_download_input_planar(fftup_plan* plan, uint32_t slot, void* planes);
/* job accounting (batched / multi-GPU runs): 64-bit wrapping sum of the 32-bit words of WHATEVER output slot `slot` holds --
 * the dense [3][uH][uW] float / half planes, or the interleaved 8-bit image [uH][uW][3] of a plan with
 * fftup_info.u8_store == 1 -- computed on the device: a frame's fingerprint without moving the frame over PCIe.  Sums over
 * the frames of a job do not depend on which rank or thread processed which frame; they are comparable only between plans
 * of the same precision and the same u8_store. */
FFTUP_API int fftup_output_checksum(fftup_plan* plan, uint32_t slot, uint64_t* sum);

/* Host-streamed batches (replaces the blocking transferDataFromCPU / transferDataToCPU + the two CPU
 * conversion loops of VR:1636-1748 for the batched mode, VR:1621-1760).  fftup_submit_rgb8 enqueues one whole
 * frame -- H2D copy, uint8 -> float conversion, the frame's kernels, float -> uint8 conversion, D2H copy -- and
 * returns at once with a ticket; up to `ring` frames are in flight, copies of one frame overlap the kernels of
 * its neighbours (each frame runs start to end on one of the plan's streams, consecutive frames on different ones).  A submit that finds its ring slot
 * still busy first waits for that slot's frame.  fftup_wait(ticket) returns when rgb_out of that submission is
 * complete; fftup_drain waits for everything submitted.  For the copies to be asynchronous both host buffers
 * must be page-locked: allocate them with fftup_host_alloc (pageable memory works, the copies then block).
 * Threads: fftup_submit_rgb8 / fftup_wait / fftup_drain of ONE plan may be called from several host threads at once (a
 * pool of PNG decode/encode workers feeding one plan per GPU -- plan creation is serialised by the HIP runtime, ~20 ms per
 * plan, so sixty-four plans of sixty-four threads cost seconds where one shared plan costs none); tickets are global to the plan.
 * Every other entry point needs one thread per plan at a time, as in the reference (one application per host thread). */
FFTUP_API void* fftup_host_alloc(size_t bytes);      /* NULL on failure (fftup_last_error) */
FFTUP_API void fftup_host_free(void* ptr);
FFTUP_API int fftup_submit_rgb8(fftup_plan* plan, const uint8_t* rgb_in, size_t in_stride_bytes, uint8_t* rgb_out,
                                size_t out_stride_bytes, uint64_t* ticket);
FFTUP_API int fftup_wait(fftup_plan* plan, uint64_t ticket);
FFTUP_API int fftup_drain(fftup_plan* plan);

/* The frame leaves the GPU as a finished PNG (round 4; replaces stbi_write_png's work, VR:1754, for the batched mode): like
 * fftup_submit_rgb8, but the 8-bit image stays on the device, where the PNG row filters (the reference writer's minimum-sum
 * heuristic), a Huffman-only deflate stream and its Adler-32 are computed (csrc/kernels_png.hpp); fftup_wait_png copies the
 * stream -- 14 MB instead of 25 MB of pixels for a 4096x2048 frame -- into png_out, frames it (signature, IHDR, IDAT, IEND,
 * CRCs) and returns the file's size.  png_out needs fftup_png_bound(plan) bytes (page-locked for a fast copy).  With png_out
 * named at submission already (a 16-byte aligned buffer of fftup_host_alloc; NULL: not yet) the GPU writes the stream into it
 * itself, sized by the count it knows, and fftup_wait_png(.., the same buffer, ..) only waits, adds the framing and the CRC --
 * no size round trip through the host: several frames of one thread stream back to back.  A ticket of
 * fftup_submit_png must be collected by fftup_wait_png: its ring slot stays with it until then.  Submissions (fftup_submit_png
 * or fftup_submit_rgb8, any thread) take the next slot that holds no uncollected stream -- so threads that keep tickets open
 * while they submit cannot wait for each other in a circle as long as fewer than `ring` streams are uncollected in total; with
 * every slot held a submission waits for a collector -- another thread's fftup_wait_png (one thread submitting, another
 * collecting, more frames than slots: the submission waits) -- unless every uncollected stream is the submitting thread's own
 * AND no other thread has ever collected on this plan, which would wait forever: after a bounded wait that call fails with
 * FFTUP_E_WOULD_BLOCK (with the default ring of 1 and one thread: collect each ticket before the next submission).
 * fftup_wait_png: a device error or FFTUP_E_OVERFLOW voids the ticket and frees its slot; a caller's error (capacity too
 * small, a buffer other than the one named at submission) leaves the stream on the device and the ticket collectable.
 * -p 0 and -p 2 plans whose stream bound fits one
 * IDAT chunk (2^31 - 1 bytes: FFTUP_E_UNSUPPORTED_SIZE beyond); thread-safe like fftup_submit_rgb8 / fftup_wait. */
FFTUP_API size_t fftup_png_bound(fftup_plan* plan);
FFTUP_API int fftup_submit_png(fftup_plan* plan, const uint8_t* rgb_in, size_t in_stride_bytes, uint8_t* png_out, size_t capacity,
                               uint64_t* ticket);
FFTUP_API int fftup_wait_png(fftup_plan* plan, uint64_t ticket, uint8_t* png_out, size_t capacity, size_t* png_bytes);

/* EXTENSION: frames that never leave the GPU.  fftup_execute_device runs the plan on CALLER-OWNED device memory: frame i reads the
 * W x H image in[i] and writes the uW x uH image out[i].  No ring slot is read or written (fftup_download_planar / _rgb8 /
 * fftup_output_checksum of a slot keep returning what the last fftup_execute / _ring / submit left there); after the call
 * fftup_download_presharpen returns the tap of the call's last frame.  Every plan kind and precision is accepted.
 * Detect the feature by this symbol; fftup_version(), FFTUP_ABI_VERSION, fftup_config and fftup_info are unchanged.
 *
 * Formats.  FFTUP_FMT_RGB8: interleaved 8-bit RGB, as fftup_upload_rgb8 / fftup_download_rgb8 take and give it (input: the
 * conversion of VR:1636-1688, in the row kernel with FFTUP_FLAG_FUSE_U8_LOAD; output: u8 = trunc(255 x), saturating unless
 * FFTUP_FLAG_U8_WRAP).  FFTUP_FMT_PLANAR: 3 planes in the plan's storage type, as fftup_upload_planar / fftup_download_planar.
 * The results are, byte for byte, those of upload -> fftup_execute(1) -> download on the same plan.
 *
 * Ordering.  The call is asynchronous to the host and never synchronises it.  All of its work starts after everything enqueued
 * on `stream` before the call, and everything enqueued on `stream` after the call returns starts after the call's last kernel (one
 * event recorded on `stream` that every lane used waits for; one completion event per lane used that `stream` waits for).  The
 * caller keeps the memory of `in` and `out` alive and untouched until `stream` has passed that point; the descriptor arrays
 * themselves are read before the call returns.  Consecutive frames alternate on the plan's FFTUP_STREAMS lanes exactly as in
 * fftup_execute_ring, so a batch overlaps like that call's.  One host thread per plan at a time, as for fftup_execute; entry
 * points of the same plan called later are ordered behind the call.
 *
 * In place, or through one staging kernel (the output bytes are the same either way):
 *   PLANAR input  -- read in place by the frame's first kernel, with the caller's strides, on every plan kind: all first kernels
 *                    load single elements at 64-bit offsets, so `data` only has to be a multiple of the element size (strides
 *                    are, by the rules below).  Otherwise one strided gather into a per-lane staging buffer.
 *   RGB8 input    -- read in place by the row kernel on plans with FFTUP_FLAG_FUSE_U8_LOAD (-p 0 / -p 2), any address and
 *                    stride; otherwise one conversion kernel from the caller's rows into the per-lane staging planes.
 *   PLANAR output -- written in place by the frame's last kernel when the image is dense (row_stride_bytes = uW * element size,
 *                    plane_stride_bytes = uW * uH * element size) and `data` is 16-byte aligned (the last kernels store up to 16
 *                    bytes at once).  Otherwise the frame goes to a per-lane scratch image and one strided scatter.
 *   RGB8 output   -- fftup_info.u8_store == 1: written in place by the fused kernel when the rows are dense (3 * uW bytes),
 *                    through the lane scratch and a strided byte copy otherwise.  Other plans: the conversion kernel writes the
 *                    caller's rows, any stride, from the lane scratch image.
 * Staging and scratch buffers are allocated by the first call that needs them and freed with the plan.
 * Containment: the library never writes a byte of caller memory outside the `height` rows of `width` pixels a descriptor names --
 * no row padding, no plane padding, nothing in front of `data` or behind the last row.
 *
 * Validation happens before any launch; on failure nothing is enqueued.  FFTUP_E_INVALID_ARG (fftup_last_error names the rule
 * and the image): a null pointer; n_frames == 0; an unknown format; a row stride below one row or, PLANAR, a stride that is not a
 * multiple of the element size or a plane stride below height * row_stride_bytes; PLANAR output on a plan with
 * fftup_info.u8_store == 1 (it has no planes: the rule of fftup_download_planar); `data` that hipPointerGetAttributes does not
 * report as device memory of the plan's device (host pointers, other devices).  No check reads or writes the memory itself.
 * The memory must come from the HIP runtime this library is linked to: a process that holds a second copy of the runtime (a
 * Python wheel that bundles its own libamdhip64, say) cannot hand that copy's pointers or streams to this call. */
enum { FFTUP_FMT_RGB8 = 0,     /* interleaved 8-bit RGB, rows of row_stride_bytes >= 3*width; plane_stride_bytes ignored */
       FFTUP_FMT_PLANAR = 1 }; /* 3 planes in the plan's storage type (float -p 0, double -p 1, IEEE half -p 2) */
typedef struct fftup_device_image {
    void*    data;               /* device memory of the plan's device */
    uint32_t format;             /* FFTUP_FMT_* */
    size_t   row_stride_bytes;   /* >= one row; PLANAR: a multiple of the element size */
    size_t   plane_stride_bytes; /* PLANAR: >= height*row_stride_bytes, a multiple of the element size */
} fftup_device_image;

/* n_frames frames: frame i reads in[i] (W x H) and writes out[i] (uW x uH).  Asynchronous to the host. */
FFTUP_API int fftup_execute_device(fftup_plan* plan, const fftup_device_image* in, const fftup_device_image* out,
                                   uint32_t n_frames, void* stream /* hipStream_t; NULL = the default stream */);

/* EXTENSION: a view per frame -- a zoom or pan across a clip, one sub-pixel offset per frame, a viewport that follows a cursor.
 * fftup_execute_device_views is fftup_execute_device on a VIEW plan (fftup_plan_create_view, with or without FFTUP_FLAG_MIRROR)
 * with frame i computed with views[i]: everything documented above holds -- formats, in-place rules, containment, ordering,
 * validation before any launch, no host synchronisation.  Frame i's result is what a plan created with views[i] gives for that
 * frame, up to the rounding of the chirp tables: they are built ON THE DEVICE, by one kernel (view_tables) enqueued on the frame's
 * lane ahead of its four kernels, in fp64 with compensated phases (csrc/view_phase.hpp), every entry within one fp32 rounding step
 * of the host tables fftup_plan_set_view uploads.  Each lane owns a table set (allocated by the first call, freed with the plan);
 * stream order alone protects it.  A frame whose span on an axis is the one its lane's tables were last built for rebuilds only the
 * origin's table on that axis (a pan).  The plan's own view is untouched: fftup_plan_set_view, fftup_plan_describe,
 * fftup_plan_info and later fftup_execute / ring / submit calls stay as they were; fftup_download_presharpen returns the call's
 * last frame.  The `views` array is read before the call returns.
 * FFTUP_E_INVALID_ARG, before anything is enqueued, beyond fftup_execute_device's: `views` is null; the plan is not a view plan;
 * a view breaks a rule of fftup_plan_set_view (fftup_last_error names the frame index and the rule).
 * Detect the feature by this symbol; fftup_version() and FFTUP_ABI_VERSION are unchanged. */
FFTUP_API int fftup_execute_device_views(fftup_plan* plan, const fftup_device_image* in, const fftup_device_image* out,
                                         const fftup_view* views, uint32_t n_frames, void* stream);

/* TEST TAP, in the spirit of fftup_download_presharpen: the tables lane `lane` (< FFTUP_STREAMS) last built for `axis` (0: x, 1: y)
 * in fftup_execute_device_views.  Interleaved (re, im) floats: pre 2 (2 kmax + 1), post 2 out_length, bhat 2 L (L: the axis'
 * convolution length, fftup_plan_describe); a null pointer skips that table or kmax.  Waits for the lane's stream first.
 * FFTUP_E_INVALID_ARG: not a view plan, a lane that has built no tables yet, a bad lane or axis. */
FFTUP_API int fftup_download_view_tables(fftup_plan* plan, uint32_t lane, uint32_t axis, float* pre, float* post, float* bhat, int32_t* kmax);

/* The device-side siblings of fftup_host_alloc, for hosts without HIP bindings (ctypes, tests): device memory and streams of the
 * runtime this library uses.  fftup_device_alloc: NULL on failure (fftup_last_error).  fftup_device_copy: kind 0 host to device,
 * 1 device to host, 2 device to device; enqueued on `stream` (NULL = the default stream), then waits for `stream`: blocking.
 * fftup_stream_create: a non-blocking stream of `device` (FFTUP_E_NO_DEVICE: bad device id); fftup_stream_destroy waits for it first. */
FFTUP_API void* fftup_device_alloc(int device, size_t bytes);
FFTUP_API void fftup_device_free(void* ptr);
FFTUP_API int fftup_device_copy(void* dst, const void* src, size_t bytes, int kind, void* stream);
FFTUP_API int fftup_stream_create(int device, void** stream);
FFTUP_API int fftup_stream_destroy(void* stream);

/* EXTENSION: shift estimates -- what a view per frame needs to stabilise a clip.  An ALIGNER is a small object beside the plan: for
 * pairs of frames in device memory, fftup_align_shifts estimates the translation between ref[i] and cur[i] by band-limited
 * phase-only correlation with a sub-pixel refinement, entirely on the GPU.  dx, dy are in input pixels, cur(x, y) ~ ref(x - dx, y - dy):
 * a view of cur at origin + (dx, dy) shows what the same view of ref shows at origin.
 * Detect the feature by these symbols; fftup_version() and FFTUP_ABI_VERSION are unchanged.
 *
 * Geometry (arithmetic on the configuration, decided before any device access; fftup_last_error names the rule;
 * fftup_align_get_info reports it).  The frames are box-averaged over d x d pixels and a centred window of n_x x n_y decimated
 * pixels is correlated: crop_x = (W - n_x d) / 2, crop_y alike.  decimate = 0: the smallest d of 1, 2, 4, 8 for which the largest
 * powers of two <= W / d and <= H / d are both <= 1024 (none: 8, the window capped at 1024); window = 0: those powers of two.
 * FFTUP_E_INVALID_ARG: a window that is not a power of two in [16, 1024] or with window * d above the frame, d not 1, 2, 4 or 8,
 * a frame below 16 decimated pixels on an axis, band outside (0, 1], upsample outside [4, 64]; FFTUP_E_UNSUPPORTED_PRECISION:
 * precision 1.  band_kx = floor(band n_x / 2), band_ky alike; K = the number of bins k (signed, -n/2 <= k < n/2 per axis) with
 * |k_x| <= band_kx and |k_y| <= band_ky.
 *
 * The estimate, per pair (fp32 arithmetic, the sums of step 5 in fp64; tests/align_oracle.py restates it in fp64):
 *   1. luma = 0.2126 R + 0.7152 G + 0.0722 B (RGB8: code / 255; PLANAR: the stored value), box mean over d x d, crop, times the
 *      separable window w[n] = 1/2 - 1/2 cos(2 pi (n + 1/2) / N): a (ref) and b (cur).
 *   2. ONE complex transform Z = DFT2(a + i b); A[k] = (Z[k] + conj Z[-k]) / 2, B[k] = (Z[k] - conj Z[-k]) / 2i.
 *   3. P = B conj(A), R = P / |P|; R = 0 outside the band and where |P| <= 1e-9 |P[0,0]|.  P[0,0] = 0 -- a frame that is black in
 *      the window: R = 0 everywhere (what step 2 leaves in the black frame's transform is rounding, not signal), and steps 4-6
 *      give dx = dy = -d, peak = peak_coarse = 0 by the tie rule alone.
 *   4. r = Re IDFT2(R); coarse peak p = argmax over the n_x x n_y grid (lowest row-major index on a tie),
 *      peak_coarse = r_max n_x n_y / K (identical frames: 1).
 *   5. r(u, v) = (1 / n_x n_y) Re sum_k R[k] exp(2 pi i (k_x u / n_x + k_y v / n_y)) on the (2 kappa + 1)^2 points
 *      (p_x + i / kappa, p_y + j / kappa), |i|, |j| <= kappa; argmax (same tie rule); per axis the vertex delta of the parabola
 *      through the maximum and its two fine neighbours (0 on the grid's edge or for a zero denominator);
 *      peak = the fine maximum times n_x n_y / K.
 *   6. s = p + (i + delta) / kappa, wrapped to [-n/2, n/2) per axis; dx = d s_x, dy = d s_y.
 *
 * Ordering and containment, as fftup_execute_device: everything is enqueued on `stream`, the host is never synchronised, the
 * descriptor arrays are read before the call returns; the frames are only read; exactly n_pairs * sizeof(fftup_shift) bytes of
 * shifts_device are written.  ref[i] and cur[i] may alias other pairs' images (a fixed reference, consecutive frames).  The
 * buffers of max_batch pairs are allocated at creation, fftup_align_shifts allocates nothing; a longer call runs in chunks, in
 * stream order.  One host thread per aligner at a time.
 * Validation happens before any launch: FFTUP_E_INVALID_ARG for null pointers, n_pairs == 0 and every descriptor rule of
 * fftup_execute_device (format, strides, device memory of the aligner's device -- shifts_device too, which must be a multiple of 4). */
typedef struct fftup_align_config {
    uint32_t width, height;      /* the frames' size */
    uint32_t precision;          /* element type of FFTUP_FMT_PLANAR frames: 0 float, 2 IEEE half (1: FFTUP_E_UNSUPPORTED_PRECISION) */
    int32_t  device;
    uint32_t window_w, window_h; /* correlation window in decimated pixels: powers of two in [16, 1024]; 0 = automatic */
    uint32_t decimate;           /* d: box-average d x d input pixels first; 1, 2, 4 or 8; 0 = automatic */
    float    band;               /* share of each axis' Nyquist range that is correlated, (0, 1]; 0 = 0.5 */
    uint32_t upsample;           /* kappa: fine-grid points per window pixel, 4..64; 0 = 32 */
    uint32_t max_batch;          /* pairs whose buffers are held; 0 = 16; longer calls run in chunks */
} fftup_align_config;
typedef struct fftup_shift { float dx, dy, peak, peak_coarse; } fftup_shift;
typedef struct fftup_align fftup_align;
typedef struct fftup_align_info {
    uint32_t window_w, window_h, decimate, crop_x, crop_y, upsample, band_kx, band_ky, num_kernels;
    uint64_t device_bytes;
    char     kernel_names[8][64];
} fftup_align_info;
FFTUP_API int fftup_align_create(fftup_align** out, const fftup_align_config* cfg);
FFTUP_API void fftup_align_destroy(fftup_align* a);
FFTUP_API int fftup_align_get_info(const fftup_align* a, fftup_align_info* info);
FFTUP_API int fftup_align_shifts(fftup_align* a, const fftup_device_image* ref, const fftup_device_image* cur,
                                 uint32_t n_pairs, fftup_shift* shifts_device, void* stream /* hipStream_t; NULL = the default stream */);

/* EXTENSION: views moved by shifts in DEVICE memory -- the estimates above reach the views without a host copy.
 * fftup_execute_device_views_shifted is fftup_execute_device_views with ONE change: frame i is computed at views[i] with its origin
 * moved by (dx, dy) of shifts_device[i].  The shift is read on the GPU, by the frame's own table kernel (view_tables) when it runs;
 * the host never reads it and never waits for it, so the output of fftup_align_shifts or fftup_shift_path enqueued on `stream`
 * before this call is consumed without a synchronisation: all of the call's work starts after everything enqueued on `stream`
 * before the call, as for fftup_execute_device.
 * Per axis origin_i = views[i].origin + (double)shift -- ONE IEEE double addition of the fp32 value widened to double -- and the
 * tables follow from origin_i by the arithmetic of csrc/view_phase.hpp as for any view.  A dx or dy that is not finite counts as 0
 * on that axis, independently of the other axis; peak and peak_coarse are not read.  Everything the host derives from a view
 * (the bins and spectrum columns kept, the sharpen constant, which tables a lane rebuilds, the rules of fftup_plan_set_view) depends
 * on the span alone and is taken from views[i]: no shift can break a rule.  The result is byte for byte what
 * fftup_execute_device_views gives for views whose origins the host moved by the same fp32 shifts in double.
 * The caller keeps shifts_device alive and unwritten until `stream` has passed the call; exactly n_frames * sizeof(fftup_shift)
 * bytes are read there, nothing is written.  The plan's own view, fftup_plan_set_view, fftup_plan_describe, fftup_plan_info and the
 * slot paths stay as they are; fftup_download_view_tables returns what the lane last built, the shift included.
 * FFTUP_E_INVALID_ARG, before anything is enqueued: everything fftup_execute_device_views refuses; shifts_device null, not a
 * multiple of 4, or not device memory of the plan's device.
 * Detect the feature by this symbol; fftup_version() and FFTUP_ABI_VERSION are unchanged. */
FFTUP_API int fftup_execute_device_views_shifted(fftup_plan* plan, const fftup_device_image* in, const fftup_device_image* out,
                                                 const fftup_view* views, const fftup_shift* shifts_device,
                                                 uint32_t n_frames, void* stream);

/* EXTENSION: a smoothed camera path -- the second half of a stabiliser.  fftup_shift_path turns n_frames measured shifts into the
 * view offsets that follow a low-passed camera path instead of locking every frame on the reference: ONE kernel (shift_path, one
 * workgroup) on `stream`, asynchronous, no allocation, no host read; the device is the one the pointers belong to.
 * out_device == in_device is allowed (every input is read before anything is written).  No atomics: the same call gives the same
 * bytes.  All arithmetic in fp64, per axis, i = 0 .. n_frames - 1 (csrc/shift_path.hpp; tests/path_oracle.py restates it):
 *   frame i is MEASURED when in[i].peak >= min_peak (a NaN peak is not) and in[i].dx, in[i].dy are both finite.
 *   FFTUP_PATH_ABSOLUTE: in[i] is frame i against one fixed reference.  p[i] = in[i] if measured, else p[i - 1]; p[-1] = 0.
 *   FFTUP_PATH_CONSECUTIVE: in[i] is frame i against frame i - 1.  p[0] = 0 (in[0] is ignored whatever it holds),
 *     p[i] = p[i - 1] + in[i] if measured, else p[i - 1].
 *   The target path s: sigma == 0: s = 0 -- every frame locked on the reference.  Otherwise r = ceil(3 sigma),
 *     g[j] = exp(-j^2 / (2 sigma^2)), s[i] = sum_{|j| <= r} g[j] p[clamp(i + j, 0, n_frames - 1)] / sum_{|j| <= r} g[j].
 *   out[i].dx, out[i].dy = (float)(p[i] - s[i]), one rounding; out[i].peak and out[i].peak_coarse are in[i]'s, bit for bit.
 * Sign: cur(x) ~ ref(x - d), so frame i shows at origin + p[i] what frame 0 shows at origin, and at origin + p[i] - s[i] it follows
 * the smoothed camera: the offsets are what fftup_execute_device_views_shifted takes.  A path that is smooth already (p linear, away
 * from the clip's ends) gets offsets of 0.
 * FFTUP_E_INVALID_ARG (fftup_last_error names the rule), before anything is enqueued: a null pointer; n_frames == 0 or above
 * FFTUP_PATH_MAX_FRAMES; mode > 1; sigma negative, not finite or above 256; min_peak not finite; in_device or out_device not a
 * multiple of 4, not device memory, or memory of two devices.
 * Detect the feature by this symbol; fftup_version() and FFTUP_ABI_VERSION are unchanged. */
enum { FFTUP_PATH_ABSOLUTE = 0, FFTUP_PATH_CONSECUTIVE = 1, FFTUP_PATH_MAX_FRAMES = 4096 };
typedef struct fftup_path_config { uint32_t mode; float sigma; float min_peak; } fftup_path_config;
FFTUP_API int fftup_shift_path(const fftup_path_config* cfg, const fftup_shift* in_device, fftup_shift* out_device,
                               uint32_t n_frames, void* stream /* hipStream_t; NULL = the default stream */);

/* EXTENSION: rotation by three shears -- camera roll, the other half of hand shake.  A ROTATOR is a small object beside the plan,
 * like the aligner: fftup_rotate_frames turns frames in caller-owned device memory about a centre, and every resampling step is
 * the exact trigonometric interpolant of the frame.  Detect the feature by these symbols; fftup_version() and FFTUP_ABI_VERSION
 * are unchanged.
 *
 * Definition (tests/rotate_oracle.py restates it in fp64).  A frame of W x H pixels is periodic on both axes, as for every FFT
 * plan here; pixel indices are coordinates.  For a rotation (angle theta in radians, centre (c_x, c_y)) let a = -tan(theta / 2)
 * and b = sin(theta), both in double: R(theta) = Sx(a) Sy(b) Sx(a).
 *   x-shear with coefficient a, for every row y of every plane: delta = a (y - c_y), X = DFT_W(row),
 *     Y[f] = X[f] exp(-2 pi i f delta / W) for signed f with 2 |f| < W; for even W, Y[W/2] = X[W/2] cos(pi delta) -- real, as the
 *     view plans treat an even length's Nyquist bin; the new row is IDFT_W(Y), normalised by 1 / W.
 *   y-shear with coefficient b: the same on columns, delta = b (x - c_x), length H.
 *   out = x-shear(a) of y-shear(b) of x-shear(a) of in.  The two intermediate images are fp32 for every input format.
 * Meaning: content moves by the matrix [[cos theta, -sin theta], [sin theta, cos theta]] about the centre,
 * out(p) ~ in(c + R(-theta)(p - c)).  With y pointing down, a positive theta turns the picture clockwise on screen.
 * On odd lengths every factor is a unit phasor and a shear loses nothing: rotating by theta and then by -theta returns the frame
 * up to rounding.  On even lengths the Nyquist rule keeps the rows real but is not unitary: that round trip does not return the
 * Nyquist bins.
 * Wrap-around: content whose path leaves the frame during one of the three shears wraps around and shows up at the opposite
 * border, as with every periodic plan -- at large angles a good part of the frame.  Small angles plus the zoom of a stabilising
 * view keep such pixels out of the picture.  There is no padded canvas.
 *
 * Formats.  Input: FFTUP_FMT_RGB8 (code / 255) or FFTUP_FMT_PLANAR in the rotator's precision (0 float, 2 IEEE half;
 * 1: FFTUP_E_UNSUPPORTED_PRECISION).  Output: FFTUP_FMT_PLANAR in the same precision, one rounding from fp32, or FFTUP_FMT_RGB8
 * as u8 = clamp(floor(255 x + 0.5), 0, 255) -- ROUND TO NEAREST, not the trunc(255 x) of fftup_download_rgb8 and the plans' final
 * store: a rotation is an intermediate step, and with truncation theta = 0 would darken 8-bit frames by a code wherever the
 * transforms' rounding falls below an integer.  PLANAR `data` may be any address (a multiple of the element size is faster).
 *
 * Geometry (arithmetic on the configuration, decided before any device access; fftup_last_error names the rule and the axis).
 * FFTUP_E_UNSUPPORTED_SIZE: a width or height below 2, above 4096 (both kernels hold two LDS buffers of two interleaved sequences,
 * 139 KB at 4096) or with a prime factor above 7 (a rotator has no Bluestein path); odd lengths are accepted, they have no
 * Nyquist bin.  FFTUP_E_INVALID_ARG: max_batch above 64.
 *
 * Ordering, containment and validation of fftup_rotate_frames, as fftup_align_shifts: everything is enqueued on `stream`, the host
 * is never synchronised, the descriptor and rotation arrays are read before the call returns.  Nothing is allocated in the call:
 * two fp32 intermediates of max_batch frames are made at creation, a longer call runs in chunks, in stream order.  Three kernels
 * per chunk (fftup_rotate_info.kernel_names).  Exactly the named pixels of out[i] are written: row padding, plane padding and
 * guard bytes stay untouched.  out[i] may be in[i] (in place): the first pass has read the whole frame into the first
 * intermediate before the third writes; any other overlap between images of one call is the caller's responsibility.  One host
 * thread per rotator at a time.
 * Validation happens before any launch: FFTUP_E_INVALID_ARG for null pointers, n_frames == 0, every descriptor rule of
 * fftup_execute_device (format, strides, device memory of the rotator's device), an angle or centre that is not finite and
 * |theta| > pi / 2 (larger angles are a transpose or a flip plus a small angle); fftup_last_error names the frame index and the
 * rule. */
typedef struct fftup_rotate_config {
    uint32_t width, height;      /* the frames' size: each in [2, 4096] and 2,3,5,7-smooth */
    uint32_t precision;          /* element type of FFTUP_FMT_PLANAR frames: 0 float, 2 IEEE half (1: FFTUP_E_UNSUPPORTED_PRECISION) */
    int32_t  device;
    uint32_t max_batch;          /* frames whose intermediates are held, at most 64; 0 = 4; longer calls run in chunks */
} fftup_rotate_config;
typedef struct fftup_rotation { double angle, centre_x, centre_y; } fftup_rotation;   /* radians; pixels */
typedef struct fftup_rotate fftup_rotate;
typedef struct fftup_rotate_info {
    uint32_t width, height, num_kernels, max_batch;
    uint64_t device_bytes;
    char     kernel_names[4][64];
} fftup_rotate_info;
FFTUP_API int fftup_rotate_create(fftup_rotate** out, const fftup_rotate_config* cfg);
FFTUP_API void fftup_rotate_destroy(fftup_rotate* r);
FFTUP_API int fftup_rotate_get_info(const fftup_rotate* r, fftup_rotate_info* info);
FFTUP_API int fftup_rotate_frames(fftup_rotate* r, const fftup_device_image* in, const fftup_device_image* out,
                                  const fftup_rotation* rotations, uint32_t n_frames, void* stream /* hipStream_t; NULL = the default stream */);

/* EXTENSION: roll estimates -- what the rotator needs to undo camera roll.  A ROLL ESTIMATOR is a small object beside the plan, like
 * the aligner: for pairs of frames in device memory, fftup_roll_angles estimates the rotation between ref[i] and cur[i] about the
 * optical axis, entirely on the GPU, from the magnitudes of their spectra alone: a translation between the frames changes only the
 * phases and does not enter.  angle is in radians with the rotator's sign, cur ~ fftup_rotate_frames(ref, +angle): rotating cur by
 * -angle (fftup_rotate_frames_angles with gain = -1) undoes the roll.  The magnitude of a real frame's spectrum is symmetric about
 * the origin, so a roll is measured modulo pi: the answer lies in [-pi/2, pi/2).
 * Detect the feature by these symbols; fftup_version() and FFTUP_ABI_VERSION are unchanged.
 *
 * Geometry (arithmetic on the configuration, decided before any device access; fftup_last_error names the rule;
 * fftup_roll_get_info reports it).  Box mean, crop and window as for the aligner, with windows of at most 512: the transform is
 * zero-padded to 2 n_x x 2 n_y and 1024 is the longest line of the aligner's LDS transforms.  decimate = 0: the smallest d of 1, 2,
 * 4, 8 for which the largest powers of two <= W / d and <= H / d are both <= 512 (none: 8, the window capped at 512); window = 0:
 * those powers of two.  n = min(n_x, n_y); angles = 0: n_theta = n; rho_max = floor(band n) and rho_min = max(2, rho_max / 4)
 * (integer division), radii in bins of the padded transform; m_b = n_theta / 4; K = 2 m_b.
 * FFTUP_E_INVALID_ARG: a window that is not a power of two in [32, 512] or with window * d above the frame, d not 1, 2, 4 or 8, a
 * frame below 32 decimated pixels on an axis, band outside (0, 1] or with rho_max < 2, angles not a power of two in [32, 1024],
 * upsample outside [4, 64]; FFTUP_E_UNSUPPORTED_PRECISION: precision 1.
 *
 * The estimate, per pair (fp32 arithmetic, the sums of step 6 in fp64; tests/roll_oracle.py restates it in fp64):
 *   1. Step 1 of the aligner: luma, d x d box mean, centred crop, the separable half-sample Hann window: a (ref) and b (cur).
 *   2. a + i b in the top-left n_y x n_x corner of a zero array of 2 n_y x 2 n_x; ONE complex transform Z, unnormalised;
 *      A[k] = (Z[k] + conj Z[-k]) / 2, B[k] = (Z[k] - conj Z[-k]) / 2i.  Only rows 0 <= k_y <= rho_max n_y / n + 1 and columns
 *      |k_x| <= rho_max n_x / n + 1 are computed: nothing else is read.  (Without the padding the bilinear samples of step 3 carry
 *      a pattern fixed to the grid, which phase-only weighting amplifies: small angles lock onto 0.)
 *   3. M_A = log1p |A|, M_B = log1p |B|.  theta_j = pi j / n_theta, j < n_theta; for rho = rho_min .. rho_max the sample at
 *      k_x = rho cos(theta_j) n_x / n, k_y = rho sin(theta_j) n_y / n, bilinear between the four bins around it, indices modulo the
 *      padded lengths: profiles L_A[rho][j], L_B[rho][j].
 *   4. F_rho = DFT_{n_theta}(L[rho][.]); P[m] = sum_rho F^B_rho[m] conj F^A_rho[m]; R[m] = P[m] / |P[m]| for 1 <= |m| <= m_b where
 *      |P[m]| > 1e-9 max |P| over that band; R = 0 elsewhere (m = 0 too, and everywhere when the maximum is 0).
 *   5. r = Re IDFT(R) on the n_theta grid; coarse peak p = argmax (lowest index on a tie), peak_coarse = r_max n_theta / K
 *      (identical frames: 1).
 *   6. r(u) = (1 / n_theta) Re sum_m R[m] exp(2 pi i m u / n_theta) on the 2 kappa + 1 points u = p + i / kappa, |i| <= kappa;
 *      argmax (same tie rule); the vertex delta of the parabola through the maximum and its two fine neighbours (0 on the grid's
 *      edge or for a zero denominator); peak = the fine maximum times n_theta / K.
 *   7. s = p + (i + delta) / kappa, wrapped to [-n_theta / 2, n_theta / 2); angle = pi s / n_theta.  A pair of black frames:
 *      R = 0, and steps 5-7 give angle = -pi / n_theta, peak = peak_coarse = 0 by the tie rule alone.
 * Window size: a roll moves the spectrum by an angle, and the angular resolution of a window of n pixels is about 1 / n radians
 * before the fit: 128 x 128 recovers a roll within about a milliradian, 512 x 256 within half of that, 64 x 32 is a legal geometry but
 * errs by up to 20 mrad.  DESIGN.md has the figures.
 *
 * Ordering and containment, as fftup_align_shifts: everything is enqueued on `stream`, the host is never synchronised, the
 * descriptor arrays are read before the call returns; the frames are only read; exactly n_pairs * sizeof(fftup_roll_angle) bytes of
 * angles_device are written (reserved = 0).  The buffers of max_batch pairs are allocated at creation, fftup_roll_angles allocates
 * nothing; a longer call runs in chunks, in stream order.  No atomics: the same call gives the same bytes.  One host thread per
 * estimator at a time.
 * Validation happens before any launch: FFTUP_E_INVALID_ARG for null pointers, n_pairs == 0 and every descriptor rule of
 * fftup_execute_device (format, strides, device memory of the estimator's device -- angles_device too, which must be a multiple of 4). */
typedef struct fftup_roll_config {
    uint32_t width, height;      /* the frames' size */
    uint32_t precision;          /* element type of FFTUP_FMT_PLANAR frames: 0 float, 2 IEEE half (1: FFTUP_E_UNSUPPORTED_PRECISION) */
    int32_t  device;
    uint32_t window_w, window_h; /* window in decimated pixels: powers of two in [32, 512]; 0 = automatic */
    uint32_t decimate;           /* d: box-average d x d input pixels first; 1, 2, 4 or 8; 0 = automatic */
    float    band;               /* rho_max = floor(band * n), (0, 1]; 0 = 0.5 */
    uint32_t angles;             /* n_theta: angular samples over [0, pi), a power of two in [32, 1024]; 0 = min(window_w, window_h) */
    uint32_t upsample;           /* kappa: fine-grid points per angular sample, 4..64; 0 = 32 */
    uint32_t max_batch;          /* pairs whose buffers are held; 0 = 16; longer calls run in chunks */
} fftup_roll_config;
typedef struct fftup_roll_angle { float angle, peak, peak_coarse, reserved; } fftup_roll_angle;
typedef struct fftup_roll fftup_roll;
typedef struct fftup_roll_info {
    uint32_t window_w, window_h, decimate, crop_x, crop_y, upsample, n, angles, rho_min, rho_max, m_band, K, max_batch, num_kernels;
    uint64_t device_bytes;
    char     kernel_names[8][64];
} fftup_roll_info;
FFTUP_API int fftup_roll_create(fftup_roll** out, const fftup_roll_config* cfg);
FFTUP_API void fftup_roll_destroy(fftup_roll* r);
FFTUP_API int fftup_roll_get_info(const fftup_roll* r, fftup_roll_info* info);
FFTUP_API int fftup_roll_angles(fftup_roll* r, const fftup_device_image* ref, const fftup_device_image* cur,
                                uint32_t n_pairs, fftup_roll_angle* angles_device, void* stream /* hipStream_t; NULL = the default stream */);

/* EXTENSION: the rotator reads its angles on the GPU -- the estimates above reach the rotator without a host copy.
 * fftup_rotate_frames_angles is fftup_rotate_frames with ONE change: frame i is turned by
 *     theta_i = rotations[i].angle + gain * (double)angles_device[i].angle
 * about rotations[i]'s centre.  gain = -1 undoes a measured roll.  theta_i is formed on the device, by one small kernel per chunk
 * (rotate_coeffs) that writes the shear coefficients a = -tan(theta_i / 2), b = sin(theta_i) in double to a buffer made at
 * creation; the three shear kernels read them there.  The host never reads angles_device and never waits for it, so the output of
 * fftup_roll_angles enqueued on `stream` before this call is consumed without a synchronisation.  A device angle that is not finite
 * counts as 0; theta_i is clamped to [-pi/2, pi/2] (the host cannot refuse what it never reads); peak and peak_coarse are not read.
 * The result is fftup_rotate_frames' at theta_i up to the last place of tan and sin in double, which may differ between the device
 * and the host's libm.  Exactly n_frames * sizeof(fftup_roll_angle) bytes are read at angles_device, nothing is written there.
 * FFTUP_E_INVALID_ARG, before anything is enqueued: everything fftup_rotate_frames refuses (|rotations[i].angle| > pi/2 included);
 * angles_device null, not a multiple of 4, or not device memory of the rotator's device; a gain that is not finite.
 * Detect the feature by this symbol; fftup_rotate_frames, fftup_version() and FFTUP_ABI_VERSION are unchanged. */
FFTUP_API int fftup_rotate_frames_angles(fftup_rotate* r, const fftup_device_image* in, const fftup_device_image* out,
                                         const fftup_rotation* rotations, const fftup_roll_angle* angles_device, double gain,
                                         uint32_t n_frames, void* stream);

FFTUP_API const char* fftup_strerror(int code);
FFTUP_API const char* fftup_last_error(void);   /* thread-local detail of the last failure */
FFTUP_API const char* fftup_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FFTUP_H */
