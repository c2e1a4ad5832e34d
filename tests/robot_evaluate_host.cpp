// robot_evaluate_host.cpp — host twin of what the robot evaluation calls decide before they touch a GPU (TEST
// INFRASTRUCTURE).  Compiles csrc/salp_robot_params.h as plain C++ (tests/robot_evaluate_host_lib.py, the flags of
// oracle/Makefile's host twins) and exports check_evaluate_args(), the call flags and the record's word offsets of
// include/salp_robot_evaluate.h.
#include "../underwater-swimmer_rl_amd/csrc/salp_robot_params.h"

extern "C" {

// The status of check_evaluate_args(); the message goes to msg (msg_size bytes), "" when accepted.  rec is an address and
// is not dereferenced.
int salp_robot_evaluate_host_check(int64_t max_steps, int32_t horizon, uint32_t flags, uint64_t rec, int own_policy, int sampled,
                                   int gaussian, char* msg, int msg_size) {
  if (msg_size > 0) msg[0] = 0;
  return check_evaluate_args(max_steps, horizon, flags, (const void*)(uintptr_t)rec, own_policy != 0, sampled != 0, gaussian != 0,
                             msg, (size_t)msg_size);
}

// SALP_DEVICE_PTRS, SALP_ROBOT_EVAL_ACCUMULATE, SALP_ROBOT_EVAL_FIRST_EPISODE into out[0..2]
void salp_robot_evaluate_host_flags(uint32_t* out) {
  out[0] = SALP_DEVICE_PTRS; out[1] = SALP_ROBOT_EVAL_ACCUMULATE; out[2] = SALP_ROBOT_EVAL_FIRST_EPISODE;
}

// SALP_REVAL_* in the order RETURN, FIRST_RETURN, EULER_STEPS, FIRST_LENGTH, FIRST_END, EPISODES, REACHED, FIRST_EULER_STEPS,
// WORDS into out[0..8]
void salp_robot_evaluate_host_words(int32_t* out) {
  const int32_t w[9] = {SALP_REVAL_RETURN, SALP_REVAL_FIRST_RETURN, SALP_REVAL_EULER_STEPS, SALP_REVAL_FIRST_LENGTH,
                        SALP_REVAL_FIRST_END, SALP_REVAL_EPISODES, SALP_REVAL_REACHED, SALP_REVAL_FIRST_EULER_STEPS,
                        SALP_REVAL_WORDS};
  for (int k = 0; k < 9; ++k) out[k] = w[k];
}

}  // extern "C"
