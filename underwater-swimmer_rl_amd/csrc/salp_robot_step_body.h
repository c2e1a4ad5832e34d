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

  // _calculate_reward (:203-243) and termination (:171-185)
  const double dx = r.pos[0] - r.target[0], dy = r.pos[1] - r.target[1];
  const double dist = sqrt(dx * dx + dy * dy);
  const double r_track = (-dist + r.prev_dist) * 100;
  r.prev_dist = dist;
  const double ex = -(dx / (dist + 1e-6)), ey = -(dy / (dist + 1e-6));
  const double vn = sqrt(r.vw[0] * r.vw[0] + r.vw[1] * r.vw[1]);
  const double r_heading = (r.vw[0] / (vn + 1e-6)) * ex + (r.vw[1] / (vn + 1e-6)) * ey;
  double rew = r_track + 0.5 * r_heading;
  bool term = false, trunc = false;
  if (dist < 0.01) { term = true; rew += 10.0; }
  else if (dist > 5.0) { trunc = true; rew -= 5.0; }
  if (r.cycle >= P.max_cycles) trunc = true;

  float o[6];
  if (term || trunc) {
    if (final_obs && active) {
      observe_robot(r, o);
#pragma unroll
      for (int k = 0; k < 6; ++k) final_obs[i * 6 + k] = o[k];
    }
    reset_robot(r, P, genv);
  }
  if (active) {
    observe_robot(r, o);
    if (obs) {
#pragma unroll
      for (int k = 0; k < 6; ++k) obs[i * 6 + k] = o[k];
    }
    if (reward) reward[i] = (float)rew;
    if (terminated) terminated[i] = term ? 1 : 0;
    if (truncated) truncated[i] = trunc ? 1 : 0;
    if (inner_steps) inner_steps[i] = steps;
    store_robot(r, S, P, i);
  }
