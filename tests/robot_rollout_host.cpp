// robot_rollout_host.cpp — host twin of what the robot rollout calls decide before they touch a GPU (TEST
// INFRASTRUCTURE).  Compiles csrc/salp_robot_params.h as plain C++ (tests/robot_rollout_host_lib.py, the flags of
// oracle/Makefile's host twins) and exports check_rollout_args(), rollout_max_iters(), the horizon cap and the service
// periods the library is built with.
#include "../underwater-swimmer_rl_amd/csrc/salp_robot_params.h"

extern "C" {

// The status of check_rollout_args(); the message goes to msg (msg_size bytes), "" when accepted.
int salp_robot_rollout_host_check(int64_t max_steps, int32_t horizon, uint32_t flags, int has_source, int has_main_output,
                                  char* msg, int msg_size) {
  if (msg_size > 0) msg[0] = 0;
  return check_rollout_args(max_steps, horizon, flags, has_source != 0, has_main_output != 0, msg, (size_t)msg_size);
}
int salp_robot_rollout_host_max_cycles(void) { return SALP_ROBOT_MAX_ROLLOUT_CYCLES; }
int64_t salp_robot_rollout_host_max_iters(int32_t horizon, int64_t max_steps, int period) {
  return rollout_max_iters(horizon, max_steps, period);
}
int64_t salp_robot_rollout_host_max_steps(double dt) { return robot_max_steps(dt); }

// kRolloutPeriods into out (up to `room` entries); returns their number.  *shipped = kRolloutPeriod.
int salp_robot_rollout_host_periods(int32_t* out, int room, int32_t* shipped) {
  const int count = (int)(sizeof(kRolloutPeriods) / sizeof(kRolloutPeriods[0]));
  for (int k = 0; k < count && k < room; ++k) out[k] = kRolloutPeriods[k];
  if (shipped) *shipped = kRolloutPeriod;
  return count;
}

}  // extern "C"
