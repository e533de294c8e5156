// vkresample -- command-line front end of the MI355X FFT upscaler; drop-in for the VkResample binary.
//
// Mirrors the reference's process entry and per-thread pipeline (VkResample.cpp "VR"):
//   main()            VR:1795-1977   same flags, defaults, messages and exit codes
//   launchResample()  VR:1280-1780   plan once per thread, then per file: PNG decode -> upload ->
//                                    upscale x numIter -> download -> PNG encode
// All compute goes through the C ABI of include/fftup.h (HIP); PNG I/O is pngio (zlib).
// Extensions (do not change the reference behaviour when absent):
//   -alldevices   batched mode: thread t uses device (d + t) % device_count instead of all threads on -d
//   -fuseu8       the row kernel reads the uint8 image directly (README.md:31 roadmap item)
//   -fuseu8out    the last kernel stores the 8-bit image itself (FFTUP_FLAG_FUSE_U8_STORE): no float planes, no conversion launch
//   -wrapu8       u8 store wraps like the reference's C cast instead of saturating
//   -workqueue    batched mode: threads take the next unprocessed file from ONE shared counter (dynamic balancing over
//                 threads / GPUs of unequal speed) instead of the static stripe t+1, t+1+T, .. of VR:1622-1629
//   -tune         FFTUP_FLAG_TUNE_PLAN: time the alternatives for a size specialised at plan time, keep the fastest (wisdom file)
//   -overlap      FFTUP_FLAG_OVERLAP_ITERATIONS: the -n iterations alternate on the plan's streams ("Time:" = throughput; the
//                 default keeps them in order like the reference's barriers, VR:1217, vkFFT.h:7678)
//   -dct          FFTUP_FLAG_DCT: DCT-II -> zero-pad -> DCT-III instead of the periodic FFT (no wrap-around ringing at the borders)
//   -anysize      FFTUP_FLAG_ANY_SIZE: even sizes with a prime factor above 7 (up to 4096 per such length) run as Bluestein transforms
//   -oddsize      FFTUP_FLAG_ODD_SIZE: odd widths and heights, input or output (exact trigonometric resampling per axis)
//   -downscale    FFTUP_FLAG_DOWNSCALE: -u in [1/8, 1) crops the spectrum (band-limited decimation; with -dct: truncated DCT)
//   -size WxH     fftup_plan_create_size: the exact output size instead of -u, one factor per axis (each axis up, down or equal)
//   -centres      with -size: pixel centres aligned (FFTUP_ALIGN_CENTRE) instead of pixel 0 on pixel 0
//   -view ox,oy,sx,sy  with -size: fftup_plan_create_view -- the output shows the rectangle of the frame that starts at input position
//                 (ox, oy) and spans (sx, sy) input pixels: zoom, sub-pixel pan, any real ratio (the frame is periodic)
//   -mirror       with -size and -view: FFTUP_FLAG_MIRROR -- the frame is continued by its reflection instead: no wrap at the borders
//   -viewto ox,oy,sx,sy -frames K  with -size and -view: one image, K frames whose view moves from -view to -viewto, in ONE
//                 fftup_execute_device_views call on device buffers; K files, -o NAME.png -> NAME_0001.png ...
//   -stabilise    batched mode with -size [-view] [-mirror]: fftup_align_shifts estimates every frame's shift against frame 000001,
//                 fftup_execute_device_views_shifted shows each frame at the view moved by its shift, read from device memory
//   -roll         with -stabilise: fftup_roll_angles estimates every frame's roll against frame 000001, fftup_rotate_frames_angles turns
//                 the frame back by it (gain -1, the angle read in device memory), then shifts and views work on the level frames
//   -smooth SIGMA [-minpeak P]  with -stabilise: follow a smoothed camera path instead of locking on frame 000001 -- the shifts are
//                 estimated between consecutive frames, fftup_shift_path (Gaussian of SIGMA frames; frames with a peak below P hold
//                 the path) turns them into view offsets on the GPU, and the frame lines gain ` offset ox oy`
//   -rotate DEG [-rotatecentre X,Y]  single image mode: fftup_rotate_frames turns the decoded frame in device memory (three Fourier
//                 shears, 8-bit to 8-bit, in place), fftup_execute_device runs the plan on it; -rotate 0: the path without the flag
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "fftup.h"
#include "png_codec.hpp"

struct ResampleConfiguration {           // VkResampleConfiguration, VR:45-59
    const char* png_input_name = nullptr;
    const char* png_output_name = nullptr;
    float upscale = 1;
    uint32_t precision = 0;
    uint32_t numIter = 1;
    int device_id = 0;
    uint32_t fileUpload = 0;
    const char* ifolder_prefix = nullptr;
    const char* ofolder_prefix = nullptr;
    int numFiles = 0;
    int numThreads = 1;
    int threadId = 0;
    float sharpenConst = 0.2f;
    bool allDevices = false;
    uint32_t flags = 0;
    std::atomic<int>* workQueue = nullptr;   // -workqueue: next file number - 1, shared by all threads
    bool stageTimes = false;                 // -stagetimes: per-thread host time by stage (batched mode)
    bool gpuPng = false;                     // -gpupng: batched mode: the GPU delivers the finished PNG (fftup_submit_png)
    uint32_t outWidth = 0, outHeight = 0;    // -size WxH (0: none, the output size follows from -u)
    uint32_t align = FFTUP_ALIGN_CORNER;     // -centres
    bool hasView = false;                    // -view ox,oy,sx,sy (with -size)
    fftup_view view{};
    uint32_t frames = 0;                     // -viewto ox,oy,sx,sy -frames K: a clip of K views from `view` to `viewTo` (0: none)
    fftup_view viewTo{};
    bool roll = false;                       // -roll with -stabilise: every frame's roll against frame 000001 is estimated and undone first
    bool stabilise = false;                  // -stabilise: batched mode, every frame shown where frame 000001 shows the view
    bool smooth = false;                     // -smooth SIGMA: ... where a smoothed camera path shows it (fftup_shift_path)
    float smoothSigma = 0.f, minPeak = 0.f;  // -minpeak P
    double rotateDeg = 0.0;                  // -rotate DEG: single image mode, the frame is turned in device memory first (0: not at all)
    bool hasRotateCentre = false;            // -rotatecentre X,Y (default: the frame centre)
    double rotateCx = 0.0, rotateCy = 0.0;
};

// frame k of the K views of a move from a to b, t = k / (K - 1): per axis the origin linear in t, the span geometric; the ends exact
// (vkresample_amd.views_between is the same formula)
static fftup_view view_between(const fftup_view& a, const fftup_view& b, uint32_t k, uint32_t K)
{
    if (k == 0) return a;
    if (k == K - 1) return b;
    const double t = (double)k / (double)(K - 1);
    fftup_view v;
    v.origin_x = (1.0 - t) * a.origin_x + t * b.origin_x;
    v.origin_y = (1.0 - t) * a.origin_y + t * b.origin_y;
    v.span_x = a.span_x * std::pow(b.span_x / a.span_x, t);
    v.span_y = a.span_y * std::pow(b.span_y / a.span_y, t);
    return v;
}

// -rotate: the decoded frame goes to device memory, is turned there in place (fftup_rotate_frames, 8-bit to 8-bit) and runs through the
// plan by fftup_execute_device on the same stream; one blocking copy brings the result back
static int run_rotated(const ResampleConfiguration& config, fftup_plan* plan, const std::vector<uint8_t>& rgb, int width, int height, uint32_t uW, uint32_t uH,
                       std::vector<uint8_t>& result)
{
    const size_t inBytes = (size_t)width * height * 3, outBytes = (size_t)uW * uH * 3;
    fftup_rotate_config rc{};
    rc.width = (uint32_t)width; rc.height = (uint32_t)height; rc.precision = config.precision; rc.device = config.device_id; rc.max_batch = 1;
    fftup_rotate* rot = nullptr;
    int res = fftup_rotate_create(&rot, &rc);
    void* din = res == FFTUP_OK ? fftup_device_alloc(config.device_id, inBytes) : nullptr;
    void* dout = res == FFTUP_OK ? fftup_device_alloc(config.device_id, outBytes) : nullptr;
    if (res == FFTUP_OK && !(din && dout)) res = FFTUP_E_OUT_OF_MEMORY;
    if (res == FFTUP_OK) res = fftup_device_copy(din, rgb.data(), inBytes, 0, nullptr);
    const fftup_device_image in = {din, FFTUP_FMT_RGB8, (size_t)width * 3, 0}, out = {dout, FFTUP_FMT_RGB8, (size_t)uW * 3, 0};
    fftup_rotation r;
    r.angle = config.rotateDeg * 3.14159265358979323846 / 180.0;
    r.centre_x = config.hasRotateCentre ? config.rotateCx : 0.5 * (width - 1);
    r.centre_y = config.hasRotateCentre ? config.rotateCy : 0.5 * (height - 1);
    if (res == FFTUP_OK) res = fftup_rotate_frames(rot, &in, &in, &r, 1, nullptr);
    if (res == FFTUP_OK) res = fftup_execute_device(plan, &in, &out, 1, nullptr);
    result.resize(outBytes);
    if (res == FFTUP_OK) res = fftup_device_copy(result.data(), dout, outBytes, 1, nullptr);    // (ordered behind both, blocking)
    fftup_rotate_destroy(rot);
    fftup_device_free(din);
    fftup_device_free(dout);
    return res;
}

// -viewto: ONE image, K views, K files -- the whole clip is one fftup_execute_device_views call on device buffers (the image once,
// K output images); the tables of every view are built on the GPU ahead of its frame.  `-o NAME.png` gives NAME_0001.png ...
static int run_view_clip(const ResampleConfiguration& config, fftup_plan* plan, const std::vector<uint8_t>& rgb, int width, int height, uint32_t uW, uint32_t uH)
{
    const uint32_t K = config.frames;
    const size_t inBytes = (size_t)width * height * 3, outBytes = (size_t)uW * uH * 3;
    std::vector<fftup_view> views(K);
    for (uint32_t k = 0; k < K; k++) {
        views[k] = view_between(config.view, config.viewTo, k, K);
        printf("view %u: %.17g %.17g %.17g %.17g\n", k, views[k].origin_x, views[k].origin_y, views[k].span_x, views[k].span_y);
    }
    void* din = fftup_device_alloc(config.device_id, inBytes);
    void* dout = fftup_device_alloc(config.device_id, outBytes * K);
    int res = (din && dout) ? FFTUP_OK : FFTUP_E_OUT_OF_MEMORY;
    if (res == FFTUP_OK) res = fftup_device_copy(din, rgb.data(), inBytes, 0, nullptr);
    if (res == FFTUP_OK) {
        std::vector<fftup_device_image> in(K), out(K);
        for (uint32_t k = 0; k < K; k++) {
            in[k] = {din, FFTUP_FMT_RGB8, (size_t)width * 3, 0};
            out[k] = {(uint8_t*)dout + outBytes * k, FFTUP_FMT_RGB8, (size_t)uW * 3, 0};
        }
        res = fftup_execute_device_views(plan, in.data(), out.data(), views.data(), K, nullptr);
    }
    std::vector<uint8_t> host(outBytes * K);
    if (res == FFTUP_OK) res = fftup_device_copy(host.data(), dout, outBytes * K, 1, nullptr);   // (ordered behind the clip, blocking)
    fftup_device_free(din);
    fftup_device_free(dout);
    if (res != FFTUP_OK) {
        printf("Upscale failed: %s (%s)\n", fftup_strerror(res), fftup_last_error());
        return res;
    }
    char base[900];
    if (config.png_output_name) snprintf(base, sizeof base, "%s", config.png_output_name);
    else snprintf(base, sizeof base, "%d_%d_upscaled.png", width, (int)uW);
    std::string stem = base, ext;
    const size_t dot = stem.find_last_of('.'), slash = stem.find_last_of('/');
    if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) { ext = stem.substr(dot); stem.resize(dot); }
    for (uint32_t k = 0; k < K; k++) {
        char num[16];
        snprintf(num, sizeof num, "_%04u", k + 1);
        const std::string name = stem + num + ext;
        std::string err;
        if (!pngio::write_rgb8(name.c_str(), host.data() + outBytes * k, (int)uW, (int)uH, (size_t)uW * 3, err))
            printf("Could not write %s: %s\n", name.c_str(), err.c_str());
    }
    return FFTUP_OK;
}

// -stabilise: a folder of frames, frame 000001 the reference.  Every frame goes to device memory once; fftup_align_shifts estimates
// each frame's shift against the reference (one call, the aligner batches); fftup_execute_device_views_shifted renders frame k at
// the view's origin + its shift, read by the GPU from the aligner's result, so every output shows what the reference shows; one
// "frame %06d: shift dx dy peak p" line per frame, from a copy made behind the render call.  -smooth: the pairs are (frame k - 1,
// frame k), one fftup_shift_path between the estimates and the render turns them into the offsets of a smoothed path -- the lines
// gain " offset ox oy".  Estimates, path and render are enqueued on one stream with no host wait between them
static int run_stabilise(const ResampleConfiguration& config)
{
    const int N = config.numFiles;
    std::vector<uint8_t> frames, one;
    int width = 0, height = 0;
    for (int f = 0; f < N; f++) {
        char name[1024];
        int w = 0, h = 0, channels = 0;
        std::string err;
        snprintf(name, sizeof name, "%s/%06d.png", config.ifolder_prefix, f + 1);
        if (!pngio::load_rgb8(name, one, w, h, channels, err) || (f && (w != width || h != height))) {
            printf("Could not load %s: %s\n", name, err.empty() ? "its size differs from frame 000001's" : err.c_str());
            return FFTUP_E_INCOMPLETE;
        }
        if (!f) { width = w; height = h; frames.resize((size_t)N * w * h * 3); }
        memcpy(frames.data() + (size_t)f * width * height * 3, one.data(), (size_t)width * height * 3);
    }
    const uint32_t uW = config.outWidth, uH = config.outHeight;
    const size_t inBytes = (size_t)width * height * 3, outBytes = (size_t)uW * uH * 3;
    const fftup_view view = config.hasView ? config.view : fftup_view{0.0, 0.0, (double)width, (double)height};
    fftup_config cfg{};
    cfg.width = (uint32_t)width; cfg.height = (uint32_t)height; cfg.channels = 3; cfg.upscale = 1.0f;
    cfg.precision = config.precision; cfg.sharpen = config.sharpenConst; cfg.device = config.device_id; cfg.flags = config.flags; cfg.ring = 1;
    fftup_align_config acfg{};
    acfg.width = (uint32_t)width; acfg.height = (uint32_t)height; acfg.device = config.device_id;
    fftup_roll_config rcfg{};
    rcfg.width = (uint32_t)width; rcfg.height = (uint32_t)height; rcfg.device = config.device_id;
    fftup_rotate_config tcfg{};
    tcfg.width = (uint32_t)width; tcfg.height = (uint32_t)height; tcfg.device = config.device_id;
    fftup_plan* plan = nullptr;
    fftup_align* aligner = nullptr;
    fftup_roll* roller = nullptr;
    fftup_rotate* rotator = nullptr;
    int res = fftup_plan_create_view(&plan, &cfg, uW, uH, &view);
    if (res == FFTUP_OK) res = fftup_align_create(&aligner, &acfg);
    if (res == FFTUP_OK && config.roll) res = fftup_roll_create(&roller, &rcfg);
    if (res == FFTUP_OK && config.roll) res = fftup_rotate_create(&rotator, &tcfg);
    void* din = res == FFTUP_OK ? fftup_device_alloc(config.device_id, inBytes * N) : nullptr;
    void* dout = res == FFTUP_OK ? fftup_device_alloc(config.device_id, outBytes * N) : nullptr;
    void* dshift = res == FFTUP_OK ? fftup_device_alloc(config.device_id, sizeof(fftup_shift) * N) : nullptr;
    void* doffset = res == FFTUP_OK && config.smooth ? fftup_device_alloc(config.device_id, sizeof(fftup_shift) * N) : nullptr;
    void* dlevel = res == FFTUP_OK && config.roll ? fftup_device_alloc(config.device_id, inBytes * N) : nullptr;    // the de-rotated frames
    void* dangle = res == FFTUP_OK && config.roll ? fftup_device_alloc(config.device_id, sizeof(fftup_roll_angle) * N) : nullptr;
    if (res == FFTUP_OK && !(din && dout && dshift && (doffset || !config.smooth) && ((dlevel && dangle) || !config.roll))) res = FFTUP_E_OUT_OF_MEMORY;
    std::vector<fftup_shift> shifts((size_t)N), offsets((size_t)N);
    std::vector<fftup_roll_angle> angles((size_t)N);
    std::vector<uint8_t> host(res == FFTUP_OK ? outBytes * N : 0);
    if (res == FFTUP_OK) res = fftup_device_copy(din, frames.data(), inBytes * N, 0, nullptr);
    if (res == FFTUP_OK) {
        std::vector<fftup_device_image> ref((size_t)N), in((size_t)N), out((size_t)N);
        // -roll: every frame's roll against frame 000001, the frames turned back by it into `dlevel` (the angles read by the GPU);
        // shifts and the render then work on the level frames
        uint8_t* base = (uint8_t*)(config.roll ? dlevel : din);
        if (config.roll) {
            std::vector<fftup_device_image> first((size_t)N), raw((size_t)N), level((size_t)N);
            const std::vector<fftup_rotation> about((size_t)N, fftup_rotation{0.0, 0.5 * (width - 1), 0.5 * (height - 1)});
            for (int f = 0; f < N; f++) {
                first[f] = {din, FFTUP_FMT_RGB8, (size_t)width * 3, 0};
                raw[f] = {(uint8_t*)din + inBytes * f, FFTUP_FMT_RGB8, (size_t)width * 3, 0};
                level[f] = {base + inBytes * f, FFTUP_FMT_RGB8, (size_t)width * 3, 0};
            }
            res = fftup_roll_angles(roller, first.data(), raw.data(), (uint32_t)N, (fftup_roll_angle*)dangle, nullptr);
            if (res == FFTUP_OK)
                res = fftup_rotate_frames_angles(rotator, raw.data(), level.data(), about.data(), (const fftup_roll_angle*)dangle, -1.0, (uint32_t)N, nullptr);
        }
        for (int f = 0; f < N; f++) {
            ref[f] = {base + (config.smooth && f ? inBytes * (f - 1) : 0), FFTUP_FMT_RGB8, (size_t)width * 3, 0};
            in[f] = {base + inBytes * f, FFTUP_FMT_RGB8, (size_t)width * 3, 0};
            out[f] = {(uint8_t*)dout + outBytes * f, FFTUP_FMT_RGB8, (size_t)uW * 3, 0};
        }
        if (res == FFTUP_OK) res = fftup_align_shifts(aligner, ref.data(), in.data(), (uint32_t)N, (fftup_shift*)dshift, nullptr);
        if (res == FFTUP_OK && config.smooth) {
            const fftup_path_config pcfg{FFTUP_PATH_CONSECUTIVE, config.smoothSigma, config.minPeak};
            res = fftup_shift_path(&pcfg, (const fftup_shift*)dshift, (fftup_shift*)doffset, (uint32_t)N, nullptr);
        }
        const std::vector<fftup_view> views((size_t)N, view);
        const fftup_shift* moved = (const fftup_shift*)(config.smooth ? doffset : dshift);
        if (res == FFTUP_OK) res = fftup_execute_device_views_shifted(plan, in.data(), out.data(), views.data(), moved, (uint32_t)N, nullptr);
        if (res == FFTUP_OK) res = fftup_device_copy(host.data(), dout, outBytes * N, 1, nullptr);
        // (for printing only, behind the render call)
        if (res == FFTUP_OK) res = fftup_device_copy(shifts.data(), dshift, sizeof(fftup_shift) * N, 1, nullptr);
        if (res == FFTUP_OK && config.smooth) res = fftup_device_copy(offsets.data(), doffset, sizeof(fftup_shift) * N, 1, nullptr);
        if (res == FFTUP_OK && config.roll) res = fftup_device_copy(angles.data(), dangle, sizeof(fftup_roll_angle) * N, 1, nullptr);
        for (int f = 0; f < N && res == FFTUP_OK; f++) {
            printf("frame %06d: shift %.3f %.3f peak %.3f", f + 1, shifts[f].dx, shifts[f].dy, shifts[f].peak);
            if (config.smooth) printf(" offset %.3f %.3f", offsets[f].dx, offsets[f].dy);
            if (config.roll) printf(" roll %.5f rollpeak %.3f", angles[f].angle, angles[f].peak);
            printf("\n");
        }
    }
    fftup_device_free(din);
    fftup_device_free(dout);
    fftup_device_free(dshift);
    fftup_device_free(doffset);
    fftup_device_free(dlevel);
    fftup_device_free(dangle);
    fftup_roll_destroy(roller);
    fftup_rotate_destroy(rotator);
    fftup_align_destroy(aligner);
    fftup_plan_destroy(plan);
    if (res != FFTUP_OK) {
        printf("Stabilisation failed: %s (%s)\n", fftup_strerror(res), fftup_last_error());
        return res;
    }
    for (int f = 0; f < N; f++) {
        char name[1024];
        std::string err;
        snprintf(name, sizeof name, "%s/%06d.png", config.ofolder_prefix, f + 1);
        if (!pngio::write_rgb8(name, host.data() + outBytes * f, (int)uW, (int)uH, (size_t)uW * 3, err)) {
            printf("Could not write %s: %s\n", name, err.c_str());
            return FFTUP_E_INCOMPLETE;
        }
    }
    return FFTUP_OK;
}

// fftup_plan_create, fftup_plan_create_size under -size, fftup_plan_create_view under -size with -view
static int create_plan(const ResampleConfiguration& config, fftup_plan** plan, const fftup_config& cfg)
{
    if (config.hasView) return fftup_plan_create_view(plan, &cfg, config.outWidth, config.outHeight, &config.view);
    if (config.outWidth) return fftup_plan_create_size(plan, &cfg, config.outWidth, config.outHeight, config.align);
    return fftup_plan_create(plan, &cfg);
}

static bool findFlag(char** start, char** end, const std::string& flag)      // VR:1782-1784: exact token match
{
    return std::find_if(start, end, [&](char* a) { return flag == a; }) != end;
}
static char* getFlagValue(char** start, char** end, const std::string& flag)  // VR:1785-1794
{
    char** value = std::find_if(start, end, [&](char* a) { return flag == a; });
    if (value == end) return nullptr;
    value++;
    return value != end ? *value : nullptr;
}

static int devices_list()                                                     // VR:239-268
{
    const int n = fftup_device_count();
    for (int i = 0; i < n; i++) {
        char name[256] = "";
        fftup_device_name(i, name, sizeof name);
        printf("Device id: %d name: %s API:HIP\n", i, name);
    }
    return n > 0 ? 0 : FFTUP_E_NO_DEVICE;
}

// Batched mode: the host threads of one GPU share ONE plan.  The reference gives every thread its own application (VR:1959-1969)
// because a Vulkan queue submission blocks its thread; here a thread's share of the GPU work is one asynchronous
// fftup_submit_rgb8 per file (0.5 ms of device time against ~250 ms of PNG decode + encode), and plan creation is serialised
// by the HIP runtime (~20 ms each, tools/plan_create_time.py): 64 plans for 64 threads cost 2.6 s of a 3.7 s job
// (profiles/r04_zi_cli_batch.txt).  Plans are keyed by (device, width, height) -- threads whose first file has another size
// get another plan, as in the reference -- and live until main() has joined the threads.
static double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct SharedPlan { fftup_plan* plan = nullptr; fftup_info info{}; };
static std::mutex g_plans_mu;
static std::map<std::tuple<int, int, int>, SharedPlan> g_plans;
static int shared_plan(const ResampleConfiguration& config, const fftup_config& cfg, SharedPlan* out)
{
    std::lock_guard<std::mutex> lock(g_plans_mu);
    SharedPlan& sp = g_plans[std::make_tuple((int)cfg.device, (int)cfg.width, (int)cfg.height)];
    if (!sp.plan) {
        const int res = create_plan(config, &sp.plan, cfg);
        if (res != FFTUP_OK) { sp.plan = nullptr; return res; }
        fftup_plan_info(sp.plan, &sp.info);
    }
    *out = sp;
    return FFTUP_OK;
}
static void shared_plans_destroy()
{
    std::lock_guard<std::mutex> lock(g_plans_mu);
    for (auto& kv : g_plans)
        if (kv.second.plan) { fftup_drain(kv.second.plan); fftup_plan_destroy(kv.second.plan); }
    g_plans.clear();
}

static int launchResample(ResampleConfiguration config)                      // VR:1280-1780
{
    if (config.threadId == 0) printf("VkResample - FFT based upscaling\n");
    const double tStart = now_ms();
    double tDecode = 0, tSubmit = 0, tWait = 0, tEncode = 0;   // -stagetimes
    // which file (1-based number) is this thread's f-th one, 0 = none left.  Static stripe of the reference: f*T + t + 1 for
    // f < numLocalFiles (VR:1622-1629); -workqueue: whatever the shared counter hands out next.
    int numLocalFiles = 1;
    if (config.fileUpload) {                                                   // VR:1622-1625
        numLocalFiles = (int)std::ceil(config.numFiles / (float)config.numThreads);
        if ((numLocalFiles - 1) * config.numThreads + config.threadId > config.numFiles - 1) numLocalFiles--;
    }
    std::vector<int> claimed;
    auto fileAt = [&](int f) -> int {
        while ((int)claimed.size() <= f) {
            int n;
            if (config.workQueue) { n = config.workQueue->fetch_add(1) + 1; if (n > config.numFiles) n = 0; }
            else n = ((int)claimed.size() < numLocalFiles || claimed.empty()) ? (int)claimed.size() * config.numThreads + config.threadId + 1 : 0;
            claimed.push_back(n);
        }
        // static stripe with more threads than files: the reference still loads file threadId + 1 for the plan's size but
        // processes nothing (VR:1622-1629) -- the first claim names that file, the loops see none
        if (!config.workQueue && config.fileUpload && f >= numLocalFiles) return 0;
        return claimed[(size_t)f];
    };
    char fileName[1024];
    if (config.fileUpload) {
        if (config.workQueue && fileAt(0) == 0) {                              // -workqueue with more threads than files
            printf("Thread %d finished. No files left in the queue\n", config.threadId);
            return FFTUP_OK;
        }
        // (static stripe: the size comes from file threadId + 1 even when the thread has no file to process, VR:1357, 1622-1629)
        snprintf(fileName, sizeof fileName, "%s/%06d.png", config.ifolder_prefix, config.workQueue ? fileAt(0) : config.threadId + 1);   // VR:1357
    }
    else snprintf(fileName, sizeof fileName, "%s", config.png_input_name);

    std::vector<uint8_t> png_input;
    int width = 0, height = 0, channels = 0;
    std::string err;
    if (!pngio::load_rgb8(fileName, png_input, width, height, channels, err)) {
        printf("Image not found\n");                                           // VR:1364-1367
        return FFTUP_E_INCOMPLETE;
    }
    tDecode += now_ms() - tStart;
    int device = config.device_id;
    if (config.allDevices) {
        const int nd = fftup_device_count();
        if (nd > 0) device = (config.device_id + config.threadId) % nd;
    }
    fftup_config cfg{};
    cfg.width = (uint32_t)width; cfg.height = (uint32_t)height; cfg.channels = 3;
    cfg.upscale = config.upscale; cfg.precision = config.precision; cfg.sharpen = config.sharpenConst;
    cfg.device = device; cfg.flags = config.flags; cfg.ring = config.fileUpload ? 2 : 1;
    // -n N: the N iterations run in order on one stream, as the reference's one command buffer with its barriers does
    // (VR:1260-1265): "Time:" is the figure comparable with the reference's, and the plan (strip cuts included) is the same for
    // every N.  -overlap (extension, config.flags): the iterations alternate on the plan's streams -- a throughput figure.
    // the batched path below runs on the GPU's shared plan: one frame in flight per thread, sixteen slots at most
    // (a slot is busy for ~0.5 ms per frame; a thread comes back after tens of ms of codec work)
    const bool streamed = config.fileUpload && config.numIter == 1 && config.numFiles > 1;
    int sharers = config.numThreads;
    if (config.allDevices && fftup_device_count() > 0) sharers = (config.numThreads + fftup_device_count() - 1) / fftup_device_count();
    if (streamed) cfg.ring = (uint32_t)std::min(16, std::max(2, sharers));
    fftup_plan* plan = nullptr;
    fftup_info info{};
    int res;
    if (streamed) {
        SharedPlan sp;
        res = shared_plan(config, cfg, &sp);
        plan = sp.plan; info = sp.info;
    } else {
        res = create_plan(config, &plan, cfg);
        if (res == FFTUP_OK) fftup_plan_info(plan, &info);
    }
    if (res != FFTUP_OK) {
        // (the hint is appended: the message of the code stays as it is)
        const bool hint = res == FFTUP_E_UNSUPPORTED_SIZE && !(config.flags & FFTUP_FLAG_ANY_SIZE);
        const bool odd_hint = res == FFTUP_E_INVALID_ARG && !(config.flags & FFTUP_FLAG_ODD_SIZE) && strstr(fftup_last_error(), "must be even");
        printf("Plan creation failed: %s (%s)%s%s\n", fftup_strerror(res), fftup_last_error(),
               hint ? "; -anysize accepts even sizes with larger prime factors (each such length up to 4096)" : "",
               odd_hint ? "; -oddsize accepts odd widths and heights" : "");
        return res;
    }
    if (config.threadId == 0) {
        const int mb = (int)(info.device_bytes / 1024 / 1024);                 // VR:1450 (a shared plan is counted once per GPU)
        if (streamed) printf("VRAM per thread: %d MB Total: %d MB\n", mb / sharers, mb * ((config.numThreads + sharers - 1) / sharers));
        else printf("VRAM per thread: %d MB Total: %d MB\n", mb, config.numThreads * mb);
    }
    const uint32_t uW = info.out_width, uH = info.out_height;
    std::vector<uint8_t> png_output(streamed ? 0 : (size_t)uW * uH * 3);

    if (streamed) {
        // batched mode: the frame travels through the GPU's shared plan as ONE asynchronous submission (H2D,
        // kernels, D2H from/to this thread's page-locked buffers), ~1 ms between submit and wait; the thread's time is the
        // PNG codec (tens of ms per file), so the overlap that matters is between the THREADS -- one frame and one pair of
        // buffers per thread (a second pair would hide 1 ms per file and double the page-locking, which the driver serialises).
        const size_t inBytes = (size_t)width * height * 3, outBytes = (size_t)uW * uH * 3;
        const bool gpuPng = config.gpuPng && config.precision != 1;    // (-p 1: the host encodes)
        const size_t pngCap = gpuPng ? fftup_png_bound(plan) : 0;
        uint8_t* pin = (uint8_t*)fftup_host_alloc(inBytes);
        uint8_t* pout = (uint8_t*)fftup_host_alloc(gpuPng ? pngCap : outBytes);
        auto release = [&]() { fftup_host_free(pin); fftup_host_free(pout); };     // (no frame of this thread is in flight here)
        if (!pin || !pout) {
            printf("Upscale failed: %s (%s)\n", fftup_strerror(FFTUP_E_OUT_OF_MEMORY), fftup_last_error());
            release();
            return FFTUP_E_OUT_OF_MEMORY;
        }
        const double tSetup = now_ms() - tStart - tDecode;             // plan (shared: the first thread creates it) + page-locked buffers
        int f = 0;
        for (; fileAt(f) > 0; f++) {
            double t0 = now_ms();
            if (f > 0) {
                snprintf(fileName, sizeof fileName, "%s/%06d.png", config.ifolder_prefix, fileAt(f));
                int w2 = 0, h2 = 0;
                if (!pngio::load_rgb8(fileName, png_input, w2, h2, channels, err) || w2 != width || h2 != height) {
                    printf("Image not found\n");                               // VR:1631-1634
                    release();
                    return FFTUP_E_INCOMPLETE;
                }
                tDecode += now_ms() - t0;
                t0 = now_ms();
            }
            memcpy(pin, png_input.data(), inBytes);
            uint64_t ticket = 0;
            res = gpuPng ? fftup_submit_png(plan, pin, (size_t)width * 3, pout, pngCap, &ticket)
                         : fftup_submit_rgb8(plan, pin, (size_t)width * 3, pout, (size_t)uW * 3, &ticket);
            if (res != FFTUP_OK) {
                printf("Upscale failed: %s (%s)\n", fftup_strerror(res), fftup_last_error());
                release();
                return res;
            }
            double t1 = now_ms();
            tSubmit += t1 - t0;
            size_t pngBytes = 0;
            res = gpuPng ? fftup_wait_png(plan, ticket, pout, pngCap, &pngBytes) : fftup_wait(plan, ticket);
            t0 = now_ms();
            tWait += t0 - t1;
            if (res != FFTUP_OK) {
                printf("Download failed: %s (%s)\n", fftup_strerror(res), fftup_last_error());
                release();
                return res;
            }
            char outName[1024];
            snprintf(outName, sizeof outName, "%s/%06d.png", config.ofolder_prefix, fileAt(f));
            if (gpuPng) {                                           // the file arrived finished: filters, deflate, checksums
                FILE* fo = fopen(outName, "wb");
                const bool ok = fo && fwrite(pout, 1, pngBytes, fo) == pngBytes;
                if ((fo && fclose(fo) != 0) || !ok) printf("Could not write %s: write error\n", outName);
            } else if (!pngio::write_rgb8(outName, pout, (int)uW, (int)uH, (size_t)uW * 3, err))
                printf("Could not write %s: %s\n", outName, err.c_str());
            tEncode += now_ms() - t0;
        }
        const double tRel = now_ms();
        release();
        if (config.stageTimes)
            printf("Thread %d: %d files in %.0f ms: setup %.0f, decode %.0f, copy+submit %.0f, wait %.0f, encode+write %.0f, release %.0f ms\n",
                   config.threadId, f, now_ms() - tStart, tSetup, tDecode, tSubmit, tWait, tEncode, now_ms() - tRel);
        printf("Thread %d finished. Device name: %s API:HIP\n", config.threadId, info.device_name);   // VR:1773
        return FFTUP_OK;
    }
    if (config.frames) {                                                       // -viewto: single image mode only (main checks)
        res = run_view_clip(config, plan, png_input, width, height, uW, uH);
        fftup_plan_destroy(plan);
        if (res == FFTUP_OK) printf("Thread %d finished. Device name: %s API:HIP\n", config.threadId, info.device_name);
        return res;
    }
    for (int f = 0; config.fileUpload ? fileAt(f) > 0 : f < 1; f++) {
        if (f > 0) {
            snprintf(fileName, sizeof fileName, "%s/%06d.png", config.ifolder_prefix, fileAt(f));
            int w2 = 0, h2 = 0;
            if (!pngio::load_rgb8(fileName, png_input, w2, h2, channels, err) || w2 != width || h2 != height) {
                printf("Image not found\n");                                   // VR:1631-1634 (all files share one size)
                fftup_plan_destroy(plan);
                return FFTUP_E_INCOMPLETE;
            }
        }
        if (config.rotateDeg != 0.0) {                                        // -rotate: single image mode only (main checks)
            res = run_rotated(config, plan, png_input, width, height, uW, uH, png_output);
            if (res != FFTUP_OK) printf("Rotated upscale failed: %s (%s)\n", fftup_strerror(res), fftup_last_error());
            else {
                printf("VkResample rotated by %g degrees: %dx%d to %dx%d\n", config.rotateDeg, width, height, uW, uH);
                char rotName[1024];
                if (config.png_output_name) snprintf(rotName, sizeof rotName, "%s", config.png_output_name);
                else snprintf(rotName, sizeof rotName, "%d_%d_upscaled.png", width, (int)uW);
                if (!pngio::write_rgb8(rotName, png_output.data(), (int)uW, (int)uH, (size_t)uW * 3, err))
                    printf("Could not write %s: %s\n", rotName, err.c_str());
                printf("Thread %d finished. Device name: %s API:HIP\n", config.threadId, info.device_name);
            }
            fftup_plan_destroy(plan);
            return res;
        }
        res = fftup_upload_rgb8(plan, png_input.data(), (size_t)width * 3);   // pack loop + transferDataFromCPU
        double totTime = 0;
        if (res == FFTUP_OK) res = fftup_execute(plan, config.numIter, &totTime);   // performVulkanUpscale, VR:1692
        if (res != FFTUP_OK) {
            printf("Upscale failed: %s (%s)\n", fftup_strerror(res), fftup_last_error());
            fftup_plan_destroy(plan);
            return res;
        }
        if (!config.fileUpload && config.hasView)
            printf("VkResample view %g,%g+%gx%g: %dx%d to %dx%d Time: %0.3f ms\n", config.view.origin_x, config.view.origin_y, config.view.span_x, config.view.span_y,
                   width, height, uW, uH, totTime);
        else if (!config.fileUpload && config.outWidth)
            printf("VkResample exact size%s: %dx%d to %dx%d Time: %0.3f ms\n", config.align == FFTUP_ALIGN_CENTRE ? " (centres)" : "", width, height, uW, uH, totTime);
        else if (!config.fileUpload)
            printf("VkResample %0.1fx upscale: %dx%d to %dx%d Time: %0.3f ms\n", config.upscale, width, height, uW, uH, totTime);   // VR:1694
        res = fftup_download_rgb8(plan, 0, png_output.data(), (size_t)uW * 3);  // transferDataToCPU + unpack loop
        if (res != FFTUP_OK) {
            printf("Download failed: %s (%s)\n", fftup_strerror(res), fftup_last_error());
            fftup_plan_destroy(plan);
            return res;
        }
        char outName[1024];
        if (config.fileUpload) snprintf(outName, sizeof outName, "%s/%06d.png", config.ofolder_prefix, fileAt(f));
        else if (config.png_output_name) snprintf(outName, sizeof outName, "%s", config.png_output_name);
        else snprintf(outName, sizeof outName, "%d_%d_upscaled.png", width, (int)uW);   // VR:1706
        if (!pngio::write_rgb8(outName, png_output.data(), (int)uW, (int)uH, (size_t)uW * 3, err))
            printf("Could not write %s: %s\n", outName, err.c_str());
    }
    fftup_plan_destroy(plan);
    printf("Thread %d finished. Device name: %s API:HIP\n", config.threadId, info.device_name);   // VR:1773
    return FFTUP_OK;
}

int main(int argc, char* argv[])
{
    ResampleConfiguration config;
    char** B = argv;
    char** E = argv + argc;
    if (findFlag(B, E, "-h")) {
        // (first line: the reference's own banner, VR:1808, for scripts that look for it; then whose build this is)
        printf("VkResample v1.0.2 (16-01-2021). Author: Tolmachev Dmitrii\n");
        printf("(command line reproduced by the MI355X/HIP build, %s)\n", fftup_version());
        printf("PNG images only.\n");
        printf("	-h: this help\n");
        printf("	-devices: list the available GPUs\n");
        printf("	-d X: GPU to use (default 0)\n");
        printf("	-u X: upscale factor (float, or a ratio like 4/3; the upscaled sizes must factor into 2s, 3s, 5s and 7s)\n");
        printf("	-p X: specify precision (0 - single, 1 - double, 2 - half, default - single)\n");
        printf("	-s X: sharpening factor, 0.0-0.2 (default 0.2)\n");
        printf("	-n X: how many times to run the upscale; removes launch overhead from the reported time (default 1)\n");
        printf("Single image mode:\n");
        printf("	-i NAME: input png\n");
        printf("	-o NAME: output png (default <width>_<upscaled width>_upscaled.png)\n");
        printf("Batched mode:\n");
        printf("	-ifolder X: input folder; files are X/000001.png, X/000002.png, ...\n");
        printf("	-ofolder X: output folder, same naming\n");
        printf("	-numfiles X: number of images\n");
        printf("	-numthreads X: host threads, each with its own plan; thread t takes files t+1, t+1+X, ...\n");
        printf("Extensions:\n");
        printf("	-alldevices: thread t runs on GPU (d + t) %% count\n");
        printf("	-fuseu8: FFT kernel reads the 8-bit image directly\n");
        printf("	-fuseu8out: the last kernel writes the 8-bit image directly (no float planes, no conversion pass)\n");
        printf("	-wrapu8: 8-bit store wraps like the original's C cast instead of saturating\n");
        printf("	-workqueue: batched mode: threads take the next unprocessed file from one shared counter instead of the fixed stripe\n");
        printf("	-gpupng: batched mode: the GPU also encodes the PNG (row filters, Huffman-only deflate, Adler-32); the host writes the file\n");
        printf("	-stagetimes: batched mode: every thread reports its host time by stage (decode, submit, wait, encode)\n");
        printf("	-tune: sizes whose kernels are specialised at plan time: measure the alternatives once, remember the fastest\n");
        printf("	-overlap: the -n iterations overlap on several streams: 'Time:' becomes a throughput figure, not the original's serial one\n");
        printf("	-dct: DCT upscale instead of FFT: the image is not treated as periodic, no ringing at the borders (-p 0 and -p 2)\n");
        printf("	-anysize: accept even sizes that do not factor into 2,3,5,7 (each such length up to 4096; Bluestein transforms; -p 0 and -p 2, not with -dct)\n");
        printf("	-oddsize: accept odd widths and heights, e.g. 853x480 or -u 1.5 on 62x38: exact trigonometric resampling (-p 0 and -p 2, not with -dct; with -anysize: any length up to 4096)\n");
        printf("	-downscale: allow -u in [1/8, 1), e.g. -u 1/2: spectral downscale (band-limited, no aliasing; -p 0 and -p 2; with -dct: DCT downscale)\n");
        printf("	-size WxH: the exact output size instead of -u, e.g. -size 1920x1080 on 1366x768: one factor per axis, each between 1/8 and 8, up or down (exact trigonometric resampling; -p 0 and -p 2, not with -dct or -u; -anysize for lengths with prime factors above 7)\n");
        printf("	-centres: with -size: align the pixel centres, as other resizers do (default: output pixel 0 on input pixel 0)\n");
        printf("	-view OX,OY,SX,SY: with -size: show the rectangle of the image that starts at position (OX, OY) and spans SX x SY input pixels, e.g. -size 1920x1080 -view 480,270,960,540 on 1920x1080: a 2x zoom about the centre; any real numbers (sub-pixel pan, any ratio; the image is periodic; a step SX/W outside [1/64, 8] is refused; not with -centres)\n");
        printf("	-mirror: with -size and -view: continue the image by its reflection instead of periodically: no wrap-around at the borders, e.g. -size 1920x1080 -view -0.144,-0.144,1366,768 -mirror -anysize on 1366x768 (-p 0 and -p 2, not with -dct)\n");
        printf("	-viewto OX,OY,SX,SY -frames K: with -size and -view, single image mode: a clip of K frames (2 to 9999) whose view moves from -view to -viewto (position linear, span geometric); -o NAME.png gives NAME_0001.png ...; the views are printed, one 'view k: ox oy sx sy' line each\n");
        printf("	-stabilise: batched mode with -size [-view] [-mirror]: frame 000001 is the reference; every frame's shift against it is estimated on the GPU (phase correlation) and the frame is shown at the view moved by that shift; one 'frame N: shift dx dy peak p' line each; one thread, one device\n");
        printf("	-roll: with -stabilise: every frame's roll against frame 000001 is estimated on the GPU (spectral magnitudes on a polar grid) and the frame is turned back by it about its centre before its shift is estimated and the view rendered; the angle is read by the rotator in device memory; frame sizes as -rotate (2,3,5,7-smooth, at most 4096), at least 32 pixels per axis; the frame lines gain ' roll r rollpeak p' (radians)\n");
        printf("	-smooth SIGMA [-minpeak P]: with -stabilise: follow a smoothed camera path instead of locking on frame 000001: shifts between consecutive frames, accumulated and low-passed on the GPU by a Gaussian of SIGMA frames (0 to 256; 0 locks on frame 000001); frames whose peak is below P hold the path; the frame lines gain ' offset ox oy'; at most 4096 frames\n");
        printf("	-rotate DEG [-rotatecentre X,Y]: single image mode: turn the image by DEG degrees (-90 to 90, clockwise on screen) about its centre or about pixel position (X, Y) before it is resampled: three Fourier shears in device memory, exact trigonometric interpolation; the image is periodic, so corners that leave the frame come back at the opposite border; width and height up to 4096 with factors 2, 3, 5, 7 (-p 0 and -p 2)\n");
        return 0;
    }
    if (findFlag(B, E, "-devices")) return devices_list();
    if (findFlag(B, E, "-d")) {
        char* v = getFlagValue(B, E, "-d");
        if (v) sscanf(v, "%d", &config.device_id);
        else { printf("No device is selected with -d flag\n"); return 1; }
    }
    if (findFlag(B, E, "-n")) {
        char* v = getFlagValue(B, E, "-n");
        if (v) sscanf(v, "%u", &config.numIter);
        else { printf("No number is selected with -n flag\n"); return 1; }
        if (config.numIter == 0) config.numIter = 1;
    }
    if (findFlag(B, E, "-p")) {
        char* v = getFlagValue(B, E, "-p");
        if (v) sscanf(v, "%u", &config.precision);
        else { printf("No precision is selected with -p flag\n"); return 1; }
    }
    if (findFlag(B, E, "-s")) {
        char* v = getFlagValue(B, E, "-s");
        if (v) sscanf(v, "%f", &config.sharpenConst);
        else { printf("No sharpening parameter is selected with -s flag\n"); return 1; }
    }
    if (findFlag(B, E, "-size")) {
        char* v = getFlagValue(B, E, "-size");
        char tail = 0;
        if (findFlag(B, E, "-u")) { printf("-size gives the output size: it cannot be combined with -u\n"); return 1; }
        if (!v || sscanf(v, "%ux%u%c", &config.outWidth, &config.outHeight, &tail) != 2 || !config.outWidth || !config.outHeight) {
            printf("No proper output size is selected with -size flag (WxH, e.g. 1920x1080)\n");
            return 1;
        }
        if (findFlag(B, E, "-centres")) config.align = FFTUP_ALIGN_CENTRE;
        if (findFlag(B, E, "-view")) {
            char* w = getFlagValue(B, E, "-view");
            if (config.align == FFTUP_ALIGN_CENTRE) { printf("-view places the output pixels itself: it cannot be combined with -centres\n"); return 1; }
            if (!w || sscanf(w, "%lf,%lf,%lf,%lf%c", &config.view.origin_x, &config.view.origin_y, &config.view.span_x, &config.view.span_y, &tail) != 4) {
                printf("No proper view is selected with -view flag (OX,OY,SX,SY, e.g. 480,270,960,540)\n");
                return 1;
            }
            config.hasView = true;
        }
    } else if (findFlag(B, E, "-view")) {
        printf("-view needs an output size given with -size\n");
        return 1;
    } else if (findFlag(B, E, "-centres")) {
        printf("-centres needs an output size given with -size\n");
        return 1;
    } else if (findFlag(B, E, "-u")) {
        char* v = getFlagValue(B, E, "-u");
        // (VR:1883: "%f".  Extension: "-u 4/3" -- a ratio, divided in float: the nearest float of 4/3 is what makes 1920 x 1080 come out
        // as exactly 2560 x 1440 in the reference's float arithmetic; typed as a decimal it takes eight digits, 1.3333334)
        float num = 0.f, den = 0.f;
        if (v && sscanf(v, "%f/%f", &num, &den) == 2 && den != 0.f) config.upscale = num / den;
        else if (v) sscanf(v, "%f", &config.upscale);
        else printf("No proper upscale factor is selected with -u flag, default 1\n");
    } else {
        printf("No upscale factor is selected with -u flag, default 1\n");
    }
    config.allDevices = findFlag(B, E, "-alldevices");
    if (findFlag(B, E, "-fuseu8")) config.flags |= FFTUP_FLAG_FUSE_U8_LOAD;
    if (findFlag(B, E, "-fuseu8out")) config.flags |= FFTUP_FLAG_FUSE_U8_STORE;
    if (findFlag(B, E, "-wrapu8")) config.flags |= FFTUP_FLAG_U8_WRAP;
    if (findFlag(B, E, "-tune")) config.flags |= FFTUP_FLAG_TUNE_PLAN;
    if (findFlag(B, E, "-overlap")) config.flags |= FFTUP_FLAG_OVERLAP_ITERATIONS;
    if (findFlag(B, E, "-dct")) config.flags |= FFTUP_FLAG_DCT;
    if (findFlag(B, E, "-anysize")) config.flags |= FFTUP_FLAG_ANY_SIZE;
    if (findFlag(B, E, "-oddsize")) config.flags |= FFTUP_FLAG_ODD_SIZE;
    if (findFlag(B, E, "-downscale")) config.flags |= FFTUP_FLAG_DOWNSCALE;
    if (findFlag(B, E, "-mirror")) {
        if (!config.hasView) { printf("-mirror needs a view given with -size and -view\n"); return 1; }
        config.flags |= FFTUP_FLAG_MIRROR;
    }
    if (findFlag(B, E, "-viewto") || findFlag(B, E, "-frames")) {
        char* w = getFlagValue(B, E, "-viewto");
        char* k = getFlagValue(B, E, "-frames");
        char tail = 0;
        if (!findFlag(B, E, "-viewto")) { printf("-frames needs a last view given with -viewto\n"); return 1; }
        if (!config.hasView) { printf("-viewto needs a first view given with -size and -view\n"); return 1; }
        if (!findFlag(B, E, "-frames")) { printf("-viewto needs a number of frames given with -frames\n"); return 1; }
        if (findFlag(B, E, "-ifolder")) { printf("-viewto works on one image (-i): it cannot be combined with -ifolder\n"); return 1; }
        if (!w || sscanf(w, "%lf,%lf,%lf,%lf%c", &config.viewTo.origin_x, &config.viewTo.origin_y, &config.viewTo.span_x, &config.viewTo.span_y, &tail) != 4) {
            printf("No proper view is selected with -viewto flag (OX,OY,SX,SY, e.g. 480,270,960,540)\n");
            return 1;
        }
        if (!k || sscanf(k, "%u%c", &config.frames, &tail) != 1 || config.frames < 2 || config.frames > 9999) {
            printf("No proper number of frames is selected with -frames flag (2 to 9999)\n");
            return 1;
        }
    }
    config.stageTimes = findFlag(B, E, "-stagetimes");
    config.gpuPng = findFlag(B, E, "-gpupng");
    config.stabilise = findFlag(B, E, "-stabilise");
    config.roll = findFlag(B, E, "-roll");
    if (config.roll && !config.stabilise) { printf("-roll undoes camera roll under -stabilise: it cannot be used without it\n"); return 1; }
    if (findFlag(B, E, "-smooth")) {
        char* v = getFlagValue(B, E, "-smooth");
        char tail = 0;
        if (!config.stabilise) { printf("-smooth smooths the path of -stabilise: it cannot be used without it\n"); return 1; }
        if (!v || sscanf(v, "%f%c", &config.smoothSigma, &tail) != 1 || !(config.smoothSigma >= 0.f && config.smoothSigma <= 256.f)) {
            printf("No proper width is selected with -smooth flag (frames, a number from 0 to 256)\n");
            return 1;
        }
        config.smooth = true;
    }
    if (findFlag(B, E, "-minpeak")) {
        char* v = getFlagValue(B, E, "-minpeak");
        char tail = 0;
        if (!config.smooth) { printf("-minpeak sets which frames -smooth trusts: it cannot be used without it\n"); return 1; }
        if (!v || sscanf(v, "%f%c", &config.minPeak, &tail) != 1 || !std::isfinite(config.minPeak)) {
            printf("No proper peak is selected with -minpeak flag (a number, e.g. 0.1)\n");
            return 1;
        }
    }
    if (findFlag(B, E, "-rotate")) {
        char* v = getFlagValue(B, E, "-rotate");
        char tail = 0;
        if (!v || sscanf(v, "%lf%c", &config.rotateDeg, &tail) != 1 || !(config.rotateDeg >= -90.0 && config.rotateDeg <= 90.0)) {
            printf("No proper angle is selected with -rotate flag (degrees, a number from -90 to 90)\n");
            return 1;
        }
        if (findFlag(B, E, "-ifolder") || config.frames) { printf("-rotate works on one image (-i): it cannot be combined with -ifolder or -viewto\n"); return 1; }
        if (config.precision == 1) { printf("-rotate turns 8-bit frames and float or half planes: it cannot be combined with -p 1\n"); return 1; }
    }
    if (findFlag(B, E, "-rotatecentre")) {
        char* v = getFlagValue(B, E, "-rotatecentre");
        char tail = 0;
        if (!findFlag(B, E, "-rotate")) { printf("-rotatecentre names the centre of -rotate: it cannot be used without it\n"); return 1; }
        if (!v || sscanf(v, "%lf,%lf%c", &config.rotateCx, &config.rotateCy, &tail) != 2 || !std::isfinite(config.rotateCx) || !std::isfinite(config.rotateCy)) {
            printf("No proper centre is selected with -rotatecentre flag (X,Y, e.g. 959.5,539.5)\n");
            return 1;
        }
        config.hasRotateCentre = true;
    }
    if (config.stabilise) {
        // what the mode cannot serve: one line, exit code 1
        if (findFlag(B, E, "-i") || !findFlag(B, E, "-ifolder")) { printf("-stabilise works on a folder of frames (-ifolder, -ofolder, -numfiles): it cannot be combined with -i\n"); return 1; }
        if (!config.outWidth) { printf("-stabilise needs an output size given with -size (-u cannot be used)\n"); return 1; }
        if (config.frames) { printf("-stabilise follows the measured motion: it cannot be combined with -viewto\n"); return 1; }
        if (config.gpuPng) { printf("-stabilise writes its files on the host: it cannot be combined with -gpupng\n"); return 1; }
        if (config.align == FFTUP_ALIGN_CENTRE) { printf("-stabilise places the output pixels itself: it cannot be combined with -centres\n"); return 1; }
        int nt = 1;
        if (findFlag(B, E, "-numthreads")) { char* v = getFlagValue(B, E, "-numthreads"); if (v) sscanf(v, "%d", &nt); }
        if (nt > 1) { printf("-stabilise runs on one thread and one device: it cannot be combined with -numthreads above 1\n"); return 1; }
    }

    if (!findFlag(B, E, "-ifolder")) {
        config.fileUpload = 0;
        config.png_input_name = getFlagValue(B, E, "-i");
        if (!config.png_input_name) { printf("No input file is selected with -i flag\n"); return 1; }
        if (findFlag(B, E, "-o")) {
            config.png_output_name = getFlagValue(B, E, "-o");
            if (!config.png_output_name) { printf("No output file is selected with -o flag\n"); return 1; }
        }
    } else {
        config.fileUpload = 1;
        config.ifolder_prefix = getFlagValue(B, E, "-ifolder");
        if (!config.ifolder_prefix) { printf("No input folder+prefix is selected with -ifolder flag\n"); return 1; }
        config.ofolder_prefix = getFlagValue(B, E, "-ofolder");
        if (!config.ofolder_prefix) { printf("No output folder+prefix is selected with -ofolder flag\n"); return 1; }
        if (findFlag(B, E, "-numthreads")) {
            char* v = getFlagValue(B, E, "-numthreads");
            if (v) sscanf(v, "%d", &config.numThreads);
            else { printf("No numThreads is selected with -numthreads flag\n"); return 1; }
        }
        char* v = getFlagValue(B, E, "-numfiles");                // the reference leaves numFiles uninitialised when
        if (v) sscanf(v, "%d", &config.numFiles);                  // the flag is missing (quirk B10): required here
        else { printf("No numFiles is selected with -numfiles flag\n"); return 1; }
        if (config.numThreads < 1) config.numThreads = 1;
        if (config.numFiles < 1) { printf("No numFiles is selected with -numfiles flag\n"); return 1; }
    }
    if (config.stabilise) return run_stabilise(config) == FFTUP_OK ? 0 : 1;
    std::atomic<int> queue{0};
    if (config.fileUpload && findFlag(B, E, "-workqueue")) config.workQueue = &queue;
    auto timeSubmit = std::chrono::system_clock::now();
    std::vector<std::thread> threads;
    std::vector<int> results((size_t)config.numThreads, 0);
    for (int i = 0; i < config.numThreads; i++) {
        ResampleConfiguration loc = config;
        loc.threadId = i;
        threads.emplace_back([loc, i, &results]() { results[(size_t)i] = launchResample(loc); });
    }
    for (auto& t : threads) t.join();
    shared_plans_destroy();
    auto timeEnd = std::chrono::system_clock::now();
    double totTime = std::chrono::duration_cast<std::chrono::microseconds>(timeEnd - timeSubmit).count() * 0.001;
    printf("Total time: %0.3f s\n", totTime / 1000);
    // the reference returns VK_SUCCESS whatever its threads did (VR:1975); a failing thread is reported here
    for (int r : results) if (r != FFTUP_OK) return r;
    return 0;
}
