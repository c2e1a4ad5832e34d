// salp_policy_upload.h — the one declaration through which the two C ABI files share the upload of a policy's weights:
// public layout (include/salp_vec.h "Policy") -> device block (salp_policy.h).  Defined in salp_vec.hip, next to the
// relayout kernel it launches (salp_service_kernels.h); salp_robot.hip calls it for the robot's policies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace salp {

// The device side of one policy object: what policy_block_map / policy_header (salp_policy.h) were uploaded into.
struct PolicyBlock {
  float* block;        // PH_WORDS header words, then n_policies policies of `stride` words: what the kernels read
  float* pub;          // staging of the public layout [n_policies][words] for host-pointer uploads
  const int32_t* map;  // [stride]: word k of a policy in the block <- public word map[k] (-1: zero)
  int n_policies, words, stride;
};

// New weights (public layout, [n_policies][words]) into b.block on `st`.  Host pointer: copied to b.pub first and the
// stream is waited for.  Device pointer: one kernel launch on `st`, nothing allocated or waited for (capturable).
hipError_t policy_block_upload(const PolicyBlock& b, const float* weights, bool device_ptrs, hipStream_t st);

}  // namespace salp
