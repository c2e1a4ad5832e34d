// salp_robot_cycle_body.h — one breathing cycle of one robot, included inside the three kernels of salp_robot_kernels.h
// that run one: nozzle.solve_angles + Robot.set_control + Robot.step_through_cycle (robot.py:55-85, 335-358, 422-445).
//   salp_robot_step_kernel, salp_robot_step_record_kernel   through salp_robot_step_body.h (env step)
//   salp_robot_trajectory_kernel                            once per cycle of the trajectory (compare_trajectories.py)
// It reads the enclosing kernel's names: Rb r (the robot, advanced in place), P (physical parameters: the kernel
// argument in the step kernels, this lane's own copy in the trajectory kernel), the cycle's action in physical units
// `contraction` (m), `coast_time` (s), `yaw` (rad), `active` (false on padding lanes, which run no Euler step), and
// for the history kRecord, H and i.  It leaves `steps` (Euler steps of the cycle) and the locals of the cycle in scope.
// Included text rather than a function for the reason given at the top of salp_robot_step_body.h.
// The text is kept in four pieces — salp_robot_cycle_control.h, _consts.h, _start.h and salp_robot_euler_step.h — which
// salp_robot_rollout_kernel includes one by one around its own loop; here they are put together in their order.
// No include guard: included once per kernel (per cycle loop).
#include "salp_robot_cycle_control.h"
#include "salp_robot_cycle_consts.h"
#include "salp_robot_cycle_start.h"
#pragma unroll 1
  while (__any(cycle_time < total)) {
    if (cycle_time < total) {
#include "salp_robot_euler_step.h"
    }
  }
