// salp_exp.h — what the experiment builds (-DSALP_EXP_STAMPS, -DSALP_EXP_COUNT) put into the device code of the snake
// simulator.  No product build expands one of these macros to code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace salp {

// ---- in-kernel phase stamps (experiment build -DSALP_EXP_STAMPS, profiles/stamp_profile.py) ---------------------
// Shader-clock stamps (s_memtime) at a few phase boundaries of the step, accumulated per wavefront in scalar
// registers and written to a debug buffer of their own after the loop: where a wavefront's lifetime goes, stalls
// included.  No product build executes a stamp.
#ifdef SALP_EXP_STAMPS
struct StampAcc { uint32_t last; uint32_t acc[12]; };
#define SALP_STAMP_PARAM , StampAcc* stamps_ = nullptr
#define SALP_STAMP_PASS , stamps_
#define SALP_STAMP(i) do { if (stamps_) { const uint32_t now_ = (uint32_t)__builtin_amdgcn_s_memtime(); \
                                          stamps_->acc[i] += now_ - stamps_->last; stamps_->last = now_; } } while (0)
#else
#define SALP_STAMP_PARAM
#define SALP_STAMP_PASS
#define SALP_STAMP(i) do {} while (0)
#endif

#ifdef SALP_EXP_COUNT     // experiment build: event counters (never in the product)
__device__ unsigned long long salp_exp_counter[8];
#define SALP_COUNT(i, cond) do { if (cond) { if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) atomicAdd(&salp_exp_counter[i], 1ull); } } while (0)
#else
#define SALP_COUNT(i, cond) do {} while (0)
#endif

}  // namespace salp
