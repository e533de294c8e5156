// plan.hpp -- what the translation units of libfftup.so share: the plan object behind the opaque fftup_plan of include/fftup.h,
// error reporting, and the internal entry points between the units
//   plan_rules.cpp     the planner without a device: request checks and every decision of a plan (PlanGeometry, plan_rules.hpp)
//   fftup_plan.hip     plan creation on the device (tables, buffers, streams), destruction, fftup_plan_set_view, the plan-time tuner
//   fftup_info.hip     fftup_plan_describe / fftup_plan_info, error text, device enumeration
//   fftup_launch.hip   the frame's kernel launches -- the only unit that instantiates the frame kernels: one selector per pass and
//                      plan family (fftup_plan::Family) names the kernel, for the launch and for its LDS attribute alike
//   fftup_execute.hip  upload / execute / download (performVulkanUpscale, VkResample.cpp:1249-1279, and the transfers)
//   fftup_queue.hip    host-streamed frames: fftup_submit_rgb8 / fftup_wait / fftup_drain
//   fftup_png.hip      the device-side PNG encoder's host side
//   fftup_device_io.hip  frames in caller-owned device memory: fftup_execute_device, fftup_execute_device_views[_shifted] and the device / stream helpers
//   fftup_align.hip    shift estimates: the aligner object (fftup_align_*), beside the plan, and the launches of kernels_align.hpp; fftup_shift_path
//   fftup_rotate.hip   rotation by three shears: the rotator object (fftup_rotate_*), beside the plan, and the launches of kernels_rotate.hpp
//   jit.cpp            the plan-time compiler
//   jit_choose.cpp     the plan-time chooser: which factorizations a specialised plan runs (no device)
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fftup.h"
#include "bluestein_plan.hpp"
#include "fft_engine.hpp"
#include "jit.hpp"
#include "plan_rules.hpp"
#include "png_params.hpp"

using fftup::BzPlan;
using fftup::PngParams;

// ---- errors: fail() (plan_rules.hpp) + the HIP runtime's
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(_e == hipErrorOutOfMemory ? FFTUP_E_OUT_OF_MEMORY : FFTUP_E_HIP,           \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                        \
    } while (0)

// events that are destroyed on every exit path
struct EventList {
    std::vector<hipEvent_t> ev;
    ~EventList() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }
    int create(size_t n)
    {
        ev.assign(n, nullptr);
        for (auto& e : ev) {
            hipError_t r = hipEventCreate(&e);
            if (r != hipSuccess) { e = nullptr; return fail(FFTUP_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(r)); }
        }
        return FFTUP_OK;
    }
    hipEvent_t& operator[](size_t i) { return ev[i]; }
};

struct fftup_plan : PlanGeometry {   // the decisions (plan_rules.hpp) + what lives on the device
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipDeviceProp_t prop{};
    fftup_jit::Module* jit = nullptr;  // mixed == 3: the kernels specialised at plan time
    struct FourTables { float2 *tw1 = nullptr, *tw2 = nullptr; };   // roots of the two factors of a four-step split (PlanGeometry::Four)
    FourTables fourFtw, fourItw, colFtw, colItw;
    BzPlan bzW{}, bzH{}, bzUW{}, bzUH{};        // per transform: L (PlanGeometry::bzL), its radix list and the tables of a Bluestein transform
    float2 *phW = nullptr, *phH = nullptr;      // align = FFTUP_ALIGN_CENTRE: phase tables of the axes whose lengths differ, nullptr otherwise
    // view plans: the current view; per axis kmax, the smooth convolution length L (PlanGeometry::viewL) with its roots, and the
    // three chirp tables (view_tables.hpp)
    fftup_view vw{};
    struct ViewAxis { int kmax = 0; uint32_t L = 0; StagePlan planL{}; float2 *tw = nullptr, *pre = nullptr, *post = nullptr, *bhat = nullptr; };
    ViewAxis vx, vy;
    // fftup_execute_device_views, created by the first call: per lane a table set of its own (the sizes of vx / vy's), which
    // k_view_tables fills on the lane's stream ahead of each frame; span: the span whose post / bhat the lane holds on that axis
    // (0: none yet), kmax: of the tables last built; vroots: the L-th roots in double per axis, shared by the lanes
    struct ViewTabs { float2 *pre[2] = {nullptr, nullptr}, *post[2] = {nullptr, nullptr}, *bhat[2] = {nullptr, nullptr};
                      double span[2] = {0, 0}; int kmax[2] = {0, 0}; bool built = false; };
    std::vector<ViewTabs> vtabs;
    double2* vroots[2] = {nullptr, nullptr};
    bool R_valid = false;             // lanes[last_lane].R holds the last frame (a fused plan: only after the pre-sharpen tap has run)

    // device memory
    std::vector<void*> in_planar;     // per slot: planar float/half, row stride W, plane stride (W+2)*H
    std::vector<uint8_t*> in_u8;      // per slot: RGB u8 [H][W][3] (staging and fused-load source)
    std::vector<int> in_kind;         // per slot: 0 none, 1 planar valid, 2 u8 valid (fused)
    // batched mode runs consecutive frames on `nlanes` streams (the reference's -numthreads does the same with
    // several queues on one device); every lane owns its scratch spectra, its pre-sharpen image R (dense [3][uH][uW]) and the
    // event that joins it to other streams (lanes_join; timing disabled; lane 0 has one too, for fftup_execute_device, which
    // therefore keeps no event set of its own).  Lane 0 runs on the plan's own stream.
    struct Lane { hipStream_t stream = nullptr; float2 *S1 = nullptr, *S2 = nullptr; void* R = nullptr; hipEvent_t done = nullptr;
                  void* T4 = nullptr; };             // T4: the four-step rows' transposition buffer
    std::vector<Lane> lanes;
    int nlanes = 1;
    int last_lane = 0;                // the lane of the last frame whose inverse rows ran -- with R_valid, written by launch_frame alone
    std::vector<void*> out;           // per slot: dense [3][uH][uW]; behind the ring's slots the extra images of fftup_execute
    uint8_t* out_u8 = nullptr;        // staging for download_rgb8
    // host-streamed queue (fftup_submit_rgb8): created on first use
    // (png: the device-side PNG encoder's buffers of the slot, created on the first fftup_submit_png; state 1 = a stream waits for
    // its fftup_wait_png, 2 = being collected -- submissions skip such a slot, and wait on q_cv when every slot is held)
    struct PngSlot { PngParams p{}; bool ready = false; unsigned long long* meta_host = nullptr; uint32_t* parts_host = nullptr; hipEvent_t copied = nullptr;
                     int state = 0; uint64_t ticket = 0; std::thread::id owner{}; uint8_t* dest = nullptr; size_t dest_cap = 0; };
    struct QSlot { uint8_t* out_u8 = nullptr; hipEvent_t done = nullptr; PngSlot png;
                   bool used = false; uint64_t ticket = 0; };        // the latest submission that went through this slot
    std::vector<QSlot> q;
    std::atomic<uint64_t> q_next{0};   // next ticket (tickets count the plan's submissions); written under q_mu
    uint32_t q_cursor = 0;             // where the search for a free slot starts (slots are taken in turn, skipping uncollected PNG streams)
    std::mutex q_mu;                   // fftup_submit_rgb8 may be called by several host threads (codec workers sharing a plan)
    std::condition_variable q_cv;
    hipStream_t png_copy = nullptr;    // the sized D2H copies of fftup_wait_png
    int png_rpb = 0, png_nblocks = 0;  // rows per deflate block, blocks per frame
    size_t png_stream_bytes = 0;       // capacity of a slot's stream buffer
    uint32_t* png_crc_shift = nullptr; // device table of k_png_crc (created with the first PNG slot)
    bool png_foreign_collector = false; // some thread has collected (fftup_wait_png) a ticket another thread submitted; under q_mu
    float2 *twW = nullptr, *twH = nullptr, *twUW = nullptr, *twUH = nullptr;
    float2 *rotW = nullptr, *rotH = nullptr, *rotUW = nullptr, *rotUH = nullptr;    // DCT plans: exp(i pi k / 2n), k < n (mirror view plans: rotW, rotH)
    uint64_t device_bytes = 0;
    size_t r_bytes = 0;               // bytes of one pre-sharpen image
    uint64_t* d_sum = nullptr;        // fftup_output_checksum accumulator (created on first use)
    size_t in_plane_stride = 0;
    int executed = 0;

    // fftup_execute_device, created by the first call that needs them: the start event (timing disabled, unlike ev0); per lane the
    // staging planes (the in_planar layout) and the scratch image (the layout of an output slot) of the layouts that cannot run in place
    struct DeviceIO { hipEvent_t start = nullptr; std::vector<void*> stage_in, scratch_out; };
    DeviceIO dio;
    bool dev_executed = false;        // a frame of fftup_execute_device has run: the pre-sharpen tap is valid, the slots are not

    std::vector<void*> allocs;
};

// ---- fftup_plan.hip
int dev_alloc(fftup_plan* P, void** ptr, size_t bytes);           // hipMalloc owned by the plan
int view_frames_prepare(fftup_plan* P, int nl);                   // fftup_execute_device_views: the table sets of lanes [0, nl), the fp64 roots, on first use
inline DeviceFacts device_facts(const hipDeviceProp_t& prop)
{
    return {prop.sharedMemPerBlock ? prop.sharedMemPerBlock : 65536, prop.multiProcessorCount, prop.gcnArchName};
}
// the row kernel reads uint8 RGB directly (fp32 / fp16 plans only)
inline bool fuse_u8(const fftup_plan* P) { return (P->cfg.flags & FFTUP_FLAG_FUSE_U8_LOAD) && !P->dbl; }
inline int check_slot(fftup_plan* P, uint32_t slot)
{
    if (!P) return fail(FFTUP_E_INVALID_ARG, "null plan");
    if (slot >= P->ring) return fail(FFTUP_E_INVALID_ARG, "slot out of range");
    return FFTUP_OK;
}

// ---- fftup_launch.hip: everything that names a kernel (each instantiation once, in the selector of its pass and family)
// (the facts about the kernels the planner needs: plan_rules.hpp)
int kernels_allow_view_tables(const fftup_plan* P);                // ... and for k_view_tables, when the plan first runs frames with views of their own
int kernels_set_attributes(fftup_plan* P);                        // dynamic LDS sizes above 64 KB, for the kernels launch_frame's selectors give THIS plan
// One frame: its caller names all of it in a FrameRun, nothing about the frame being launched lives in the plan.  Pass: rows ..
// sharpen are the indices of fftup_profile_kernels / fftup_execute_ring_timed; presharpen_tap = the stand-alone inverse rows of
// a fused plan, from the lane's spectra into its R.  DeviceInput (fftup_execute_device): input outside the ring -- caller memory
// or a lane's staging (kind 1: planes, strides in elements; kind 2: 8-bit RGB, row stride in bytes)
enum class Pass { rows, columns, inverse, sharpen, all, presharpen_tap };
struct DeviceInput { const void* in = nullptr; int kind = 0; long in_row = 0, in_plane = 0; };
// in_slot: the ring slot the frame reads (`in`: instead of the slot); out: the image its last kernel writes -- a slot's, an extra
// one of fftup_execute, caller memory, a lane's scratch
// view: the frame's own view (fftup_execute_device_views; nullptr: the plan's) -- its tables are built on the lane's stream first
// shift: with `view`, the frame's fftup_shift in DEVICE memory (fftup_execute_device_views_shifted; nullptr: none): the table
// kernel moves the view's origin by its dx, dy when it runs, the host never reads it
struct FrameRun { int lane = 0; uint32_t in_slot = 0; void* out = nullptr; const DeviceInput* in = nullptr; Pass pass = Pass::all;
                  const fftup_view* view = nullptr; const fftup_shift* shift = nullptr; };
int launch_frame(fftup_plan* P, const FrameRun& r);               // launches, then records what the frame left: the only writer of last_lane and R_valid (but see fftup_execute)
// fftup_shift_path: k_shift_path (kernels_path.hpp) on the current device, allowed its dynamic LDS first; n, mode and sigma are the caller's, checked
int launch_shift_path(const fftup_shift* in, fftup_shift* out, uint32_t n, uint32_t mode, float sigma, float min_peak, hipStream_t st);
void launch_unpack(fftup_plan* P, uint32_t slot, hipStream_t st);                  // the host loop of VR:1636-1685 as a kernel
void launch_pack(fftup_plan* P, uint32_t slot, uint8_t* dst, hipStream_t st);      // ... and of VR:1708-1748
void launch_checksum(fftup_plan* P, uint32_t slot, hipStream_t st);                // 64-bit sum of the slot's words -> P->d_sum
// frames in caller-owned device memory (kernels_device_io.hpp)
void launch_unpack_from(fftup_plan* P, const uint8_t* rgb, size_t row_stride_bytes, void* planes, hipStream_t st);   // -> the in_planar layout
void launch_pack_to(fftup_plan* P, const void* planes, uint8_t* rgb, size_t row_stride_bytes, hipStream_t st);     // dense planes -> rows of row_stride_bytes
// `planes` x `rows` rows of row_bytes bytes between two strided layouts (strides in bytes); gran: 1, 2, 4 or 8, a power of two
// that divides both addresses, all four strides and row_bytes
void launch_copy_rows(const void* src, size_t src_row, size_t src_plane, void* dst, size_t dst_row, size_t dst_plane,
                      size_t row_bytes, uint32_t rows, uint32_t planes, int gran, hipStream_t st);

// ---- fftup_execute.hip
// fork: the lanes [first, nl) go on behind what `from` holds now (`ev` is recorded on it).  join: each of them records its `done`
// event and every stream of `into` waits for it (a stream never for itself); `rc` is the status so far, which an event failure
// does not replace
int lanes_fork(fftup_plan* P, hipEvent_t ev, hipStream_t from, int first, int nl);
int lanes_join(fftup_plan* P, int first, int nl, std::initializer_list<hipStream_t> into, int rc);
int execute_ring_impl(fftup_plan* P, uint32_t n_frames, uint32_t first_slot, double* ms_total, double* kernel_ms, uint32_t stride);

// ---- fftup_device_io.hip
// every rule of include/fftup.h for one fftup_device_image naming a `w` x `h` image of `device` (esz: bytes of a PLANAR element; u8out:
// PLANAR output is refused), the memory itself untouched.  Shared by fftup_execute_device and fftup_align_shifts (fftup_align.hip)
int check_device_image(size_t esz, bool u8out, int device, const fftup_device_image& im, const char* side, uint32_t i, uint32_t w, uint32_t h, bool is_out);

// ---- fftup_queue.hip
int submit_frame(fftup_plan* P, const uint8_t* rgb_in, size_t in_stride, uint8_t* rgb_out, size_t out_stride, bool png, uint64_t* ticket);

// ---- fftup_png.hip
void png_geometry(fftup_plan* P);                                 // rows per deflate block, stream capacity (fixed per plan)
int png_slot_init(fftup_plan* P, fftup_plan::QSlot& Q);           // the encoder's buffers of a ring slot, on first use
int png_enqueue(fftup_plan* P, fftup_plan::QSlot& Q, hipStream_t cs, uint8_t* png_dest);    // the encoder's launches behind a frame
