// salp_policy_upload.h — the declarations through which the two C ABI files share the kernels behind a policy object
// (salp_policy_object.h): the upload of its weights, public layout (include/salp_vec.h "Policy") -> device block
// (salp_policy.h), and the write of its noise step.  Defined in salp_vec.hip, next to the relayout and the noise kernel
// they launch (salp_service_kernels.h); salp_robot.hip calls them for the robot's policies.  They return the HIP status
// and know no fail(): compiled into the snake unit, it would write the wrong library's error string.
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

// The noise step in the header of `block` becomes `value` (set) or goes on by `value`: one one-thread launch on `st`.
hipError_t policy_noise_write(float* block, uint64_t value, bool set, hipStream_t st);

}  // namespace salp
