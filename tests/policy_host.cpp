// policy_host.cpp — host twin of the in-kernel policy's layout and of the set_state ranges (TEST INFRASTRUCTURE).
// Compiles the host sections of csrc/salp_policy.h and csrc/salp_params.h as plain C++ (oracle/Makefile, the flags of the
// parameter twin) and exports what salp_policy_create and salp_vec_set_state decide before they touch a GPU: the ranges of
// a policy descriptor, the map from the public weight layout to the device block, the block's header words, the byte
// counts of a policy object's allocations, and the ranges of a host snapshot.
#include <stdio.h>

#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wunused-parameter"   // make_params keeps its `seed` argument
#include "../underwater-swimmer_rl_amd/csrc/salp_params.h"
#pragma GCC diagnostic pop
#include "../underwater-swimmer_rl_amd/csrc/salp_policy.h"

using namespace salp;

extern "C" {

int salp_policy_host_header_words(void) { return PH_WORDS; }
// PH_NHIDDEN, PH_H0, PH_H1, PH_OUT, PH_STRIDE, PH_GROUP, PH_COUNT, PH_GAUSS, PH_NOISE in this order
void salp_policy_host_header_slots(int32_t slots[9]) {
  const int32_t v[9] = {PH_NHIDDEN, PH_H0, PH_H1, PH_OUT, PH_STRIDE, PH_GROUP, PH_COUNT, PH_GAUSS, PH_NOISE};
  for (int i = 0; i < 9; ++i) slots[i] = v[i];
}

// The status of check_policy_desc(); *words (nullable) the public word count, *why (nullable) the message, "" when accepted.
int salp_policy_host_check(int obs_dim, int act_dim, int kmax, int64_t n_envs, const salp_policy_desc_t* d, int gaussian,
                           int* words, const char** why) {
  const char* msg = "";
  const int rc = check_policy_desc(obs_dim, act_dim, kmax, n_envs, d, gaussian != 0, words, &msg);
  if (why) *why = msg;
  return rc;
}

// policy_block_map(): the stride; the first min(stride, capacity) entries go to map (nullable: ask for the stride first).
int salp_policy_host_map(int obs_dim, int act_dim, const salp_policy_desc_t* d, int gaussian, int32_t* map, int capacity) {
  std::vector<int32_t> m;
  const int stride = policy_block_map(obs_dim, act_dim, *d, gaussian != 0, m);
  for (int k = 0; map && k < stride && k < capacity; ++k) map[k] = m[k];
  return stride;
}

// policy_header() into the caller's salp_policy_host_header_words() words
void salp_policy_host_header(const salp_policy_desc_t* d, int stride, int64_t n_envs, int gaussian, int32_t* hd) {
  int32_t w[PH_WORDS];
  policy_header(*d, stride, n_envs, gaussian != 0, w);
  for (int i = 0; i < PH_WORDS; ++i) hd[i] = w[i];
}

// policy_bytes(): the byte counts of the block, the public staging and the map, in this order
void salp_policy_host_bytes(const salp_policy_desc_t* d, int words, int stride, uint64_t bytes[3]) {
  const PolicyBytes b = policy_bytes(*d, words, stride);
  bytes[0] = b.block; bytes[1] = b.pub; bytes[2] = b.map;
}

// The status of check_snapshot(); the message goes to msg (msg_size bytes), "" when the snapshot is accepted.
int salp_policy_host_check_snapshot(int64_t n, const double* f64, const int32_t* i32, char* msg, int msg_size) {
  if (msg_size > 0) msg[0] = 0;
  return check_snapshot(n, f64, i32, msg, (size_t)msg_size);
}

double salp_policy_host_max_angle(void) { return SALP_SET_STATE_MAX_ANGLE; }

}  // extern "C"
