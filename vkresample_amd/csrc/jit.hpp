// jit.hpp / jit.cpp -- run-time specialised plans (host side).
//
// The reference treats every 2*3*5*7-smooth size as first class because VkFFT GENERATES its shaders for the requested
// size at plan time and compiles them with glslang (vkFFT.h:4707-5189 scheduler, :6200-7700 generator, VkResample.cpp
// links glslang for it).  The MI355X-native counterpart: the register-resident kernels of kernels_pow2.hpp /
// kernels_mixed.hpp are C++ templates over the size, its radix factorisation and the upscale factor; for a plan with an
// integer or half-integer factor whose size has no ahead-of-time instantiation, fftup_plan_create
//   * picks factorizations (choose(), in a unit of its own that needs no device: jit_choose.hpp / jit_choose.cpp --
//     measured rules, a built-in table of tuner results for the MI355X, the user's wisdom file),
//   * writes two ten-line translation units that name the instantiations (make_source(): row + column kernels, and
//     fused C2R+sharpen + stand-alone C2R, which depend on the output row length only and are shared between heights),
//   * compiles it for the plan's device with hipRTC (the ROCm run-time compiler, loaded with dlopen -- no link-time
//     dependency, and without it the plan silently stays on the size-generic kernels),
//   * loads the code object, relaxes the fused kernel's register bound if it spills (load()), and launches the kernels
//     from it (launch()).
// Code objects are cached in memory and on disk ($FFTUP_CACHE_DIR, else $XDG_CACHE_HOME/fftup, else ~/.cache/fftup),
// keyed by a hash of the translation unit, the instantiated names, the compiler options, the hipRTC version and the
// kernel headers' text.
// With FFTUP_FLAG_TUNE_PLAN the plan is also timed with the alternative factorizations of its dominant kernel
// (fused_candidates(), tune_fused() in fftup_plan.hip) and the decision kept in <cache dir>/wisdom.txt.
//
// The kernel headers' text is embedded in the library at build time (kernel_sources.inc, written by
// __graft_entry__.build() from the very files the ahead-of-time kernels are compiled from) and handed to hipRTC as
// in-memory headers; $FFTUP_KERNEL_DIR overrides it with a directory (development), and a library built without the
// generated file reads csrc/ next to libfftup.so.
//
// Environment: FFTUP_JIT=0 off; FFTUP_JIT_VERBOSE=1 says why a plan fell back and what the tuner measured;
// FFTUP_HIPRTC_LIB=<libhiprtc.so>.  Experiments and tests (FFTUP_EXPERIMENT="key=value;..", see experiment()): jit_row / jit_col /
// jit_coli / jit_fused ("r0,r1,.." resp. "threads:r0,r1,..") pin a factorization (one that fails the chooser's rule,
// valid_factorization() in jit_choose.cpp, is ignored); jit_fused_opt="waves,ring" pins the fused kernel's register bound and
// ring-row placement; jit_no_builtin_wisdom; jit_dump=<file> writes the translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "jit_choose.hpp"              // Choice, choose(), the tuner's candidates, the wisdom file, experiment()

namespace fftup_jit {

enum { K_ROW_PLANAR = 0, K_ROW_U8, K_COL, K_FUSED, K_C2R_CT, K_COUNT };

// a compiled translation unit: code object + the lowered names of its kernels
struct Binary {
    std::string code;
    std::string lowered[K_COUNT];
};

// a code object loaded on one device
struct Module {
    hipModule_t mod[2] = {nullptr, nullptr};       // part 0: row + column kernels, part 1: fused C2R+sharpen + stand-alone C2R
    hipFunction_t fn[K_COUNT] = {};
    Choice choice;
    ~Module() { for (hipModule_t m : mod) if (m) (void)hipModuleUnload(m); }
};

// both translation units of a plan compiled for `arch` (cached in memory and on disk)
bool compile_both(const Choice& c, const std::string& arch, Binary b[2], std::string& err);
// ... and loaded on the current device; relaxes the fused kernel's register bound if it spills.  nullptr: err says why
Module* load(Choice c, const std::string& arch, std::string& err);

template <class Params>
inline hipError_t launch(hipFunction_t f, dim3 grid, dim3 block, size_t lds, hipStream_t st, Params p)
{
    void* args[] = {&p};
    return hipModuleLaunchKernel(f, grid.x, grid.y, grid.z, block.x, block.y, block.z, (unsigned)lds, st, args, nullptr);
}

}  // namespace fftup_jit
