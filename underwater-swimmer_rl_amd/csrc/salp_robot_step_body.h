// salp_robot_step_body.h — the body of the two step kernels of salp_robot_kernels.h (SalpRobotEnv.step,
// salp_robot_env.py:139-201: one breathing cycle per env), included inside each kernel:
//   salp_robot_step_kernel          constexpr bool kRecord = false;  RobotHistory H = {} (unused)
//   salp_robot_step_record_kernel   constexpr bool kRecord = true;   H = the kernel argument
// Its parameters are the kernels' own: P, S, act, obs, reward, terminated, truncated, final_obs, inner_steps, order.
// The cycle itself (solve_angles, set_control, the Euler loop) is salp_robot_cycle_body.h, which the trajectory
// kernel includes too.
// It is text included into the kernel rather than a __forceinline__ function: an inlined function is first
// optimised on its own and then again inside the kernel, and that moved the register allocation and the schedule
// of salp_robot_step_kernel; included text keeps its instruction stream that of the kernel before recording
// existed.
// The end of the step (reward, flags, autoreset; the stores) is salp_robot_step_finish.h and salp_robot_step_outputs.h,
// which salp_robot_rollout_kernel includes at its service points.
// No include guard: included once per kernel.
  const int64_t i0 = (int64_t)blockIdx.x * kRBlock + threadIdx.x;
  const bool active = i0 < P.n;
  // `order` (robot_schedule_* in salp_robot_kernels.h) lists the envs longest cycle first, so that the lanes of a wavefront
  // run about the same number of Euler steps; results do not depend on which lane an env runs in.
  const int64_t i = active ? (order ? (int64_t)order[i0] : i0) : (P.n - 1);
  const uint64_t genv = P.env_base + (uint64_t)i;
  Rb r;
  load_robot(r, S, P, i);

  // _rescale_action (:129-137) in fp64 (the scales: salp_robot_params.h)
  const double contraction = (double)act[i * 3 + 0] * kActContraction;
  const double coast_time = (double)act[i * 3 + 1] * kActCoast;
  const double yaw = (double)act[i * 3 + 2] * kActYaw;
#include "salp_robot_cycle_body.h"
  if constexpr (kRecord) {
    if (rec && H.len) H.len[hj] = n_samples;
  }

#include "salp_robot_step_finish.h"
  if (active) {
#include "salp_robot_step_outputs.h"
    store_robot(r, S, P, i);
  }
