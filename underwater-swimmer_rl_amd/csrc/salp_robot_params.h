// salp_robot_params.h — the parameters of a robot-simulator launch: the launch-parameter block RobotParams, the constants
// of the cycle (action scales, contract / release rates, the cycle-length cut, the schedule's bins), the list of the
// physical parameters a trajectory robot may have of its own (SALP_ROBOT_PHYS), and the host functions that derive a
// RobotParams from a salp_robot_config_t and decide what salp_robot_vec_create, salp_robot_vec_step_history,
// salp_robot_vec_trajectory, the rollout calls and the evaluation calls refuse (and the rollout kernel's service period and
// iteration bound).
//
// The header compiles in two ways, like salp_params.h and salp_fp64_math.h:
//   * with hipcc: what salp_robot.hip includes, before salp_robot_kernels.h;
//   * as plain host C++ (tests/robot_params_host.cpp): the same text with the __host__ / __device__ qualifiers dropped, so
//     that everything the host derives or refuses is under test without a GPU.
// It makes no HIP call and does not know fail(): a function that refuses returns SALP_ERR_INVALID and hands back the reason.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SALP_HOST_DEVICE __host__ __device__
#else
#define SALP_HOST_DEVICE
#endif
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/salp_robot.h"
#include "../../include/salp_robot_rollout.h"   // SALP_ROBOT_MAX_ROLLOUT_CYCLES
#include "../../include/salp_robot_evaluate.h"  // the evaluation calls' flags and SALP_REVAL_*
#include "../../include/salp_vec.h"   // SALP_OK, SALP_ERR_INVALID

// An unnamed namespace, as in salp_host.h: the kernels of salp_robot_kernels.h live in one, and RobotParams is part of their names.
namespace {

struct RobotParams {
  double dry_mass, init_length, init_width, max_contraction, density, dt, cd_min, cd_max;
  double nz_l1, nz_l2, nz_area, nz_mass, nz_gamma;
  double x_min, x_span, y_min, y_span;   // target placement, salp_robot_env.py:241-250
  int max_cycles;
  uint32_t seed_lo, seed_hi;
  uint64_t env_base;
  int64_t n, pitch;
};

constexpr double kPi = 3.141592653589793;
// _rescale_action (salp_robot_env.py:129-137): the Box action times these is contraction (m), coast time (s), nozzle yaw (rad)
constexpr double kActContraction = 0.06, kActCoast = 10.0, kActYaw = kPi / 2;
// Robot.set_control (robot.py:767, 776): the full stroke of 0.06 m is drawn in in 3 s and let go in 1.5 s
constexpr double kContractTime = 3.0, kReleaseTime = 1.5;
constexpr double kContractRate = kActContraction / kContractTime, kReleaseRate = kActContraction / kReleaseTime;   // m/s
// s; an in-Box action asks for at most 0.06 * (3 + 1.5) / 0.06 + 10 = 14.5 s.  A longer cycle is cut here (include/salp_robot.h)
constexpr double kMaxCycleTime = 14.6;
constexpr int kSchedBins = 256;   // the cycle-length schedule of salp_robot_kernels.h
// Most Euler steps of one cycle that a history may have to hold (robot_max_steps below)
constexpr int64_t kMaxHistorySteps = (int64_t)1 << 24;

// The physical parameters, one line each: X(config field, SALP_RP_* row, RobotParams member).  The copy of
// make_robot_params, the per-lane table load of salp_robot_trajectory_kernel and the check below that row k of the list
// is row k of the public table are made from it; tests/test_robot_params_host.py ties the names to robot_compare.py.
// dt, the tank and max_cycles stay the handle's and are not in it (nozzle_length3 is drawing code only).
#define SALP_ROBOT_PHYS(X) \
  X(dry_mass, SALP_RP_DRY_MASS, dry_mass) \
  X(init_length, SALP_RP_INIT_LENGTH, init_length) \
  X(init_width, SALP_RP_INIT_WIDTH, init_width) \
  X(max_contraction, SALP_RP_MAX_CONTRACTION, max_contraction) \
  X(density, SALP_RP_DENSITY, density) \
  X(drag_coefficient_min, SALP_RP_DRAG_COEFFICIENT_MIN, cd_min) \
  X(drag_coefficient_max, SALP_RP_DRAG_COEFFICIENT_MAX, cd_max) \
  X(nozzle_length1, SALP_RP_NOZZLE_LENGTH1, nz_l1) \
  X(nozzle_length2, SALP_RP_NOZZLE_LENGTH2, nz_l2) \
  X(nozzle_area, SALP_RP_NOZZLE_AREA, nz_area) \
  X(nozzle_mass, SALP_RP_NOZZLE_MASS, nz_mass) \
  X(nozzle_gamma, SALP_RP_NOZZLE_GAMMA, nz_gamma)
#define SALP_ROBOT_PHYS_ROW(field, row, member) kRobotPhysRow_##field,
enum { SALP_ROBOT_PHYS(SALP_ROBOT_PHYS_ROW) kRobotPhysCount };
#undef SALP_ROBOT_PHYS_ROW
#define SALP_ROBOT_PHYS_CHECK(field, row, member) static_assert((int)kRobotPhysRow_##field == (int)row, "parameter rows: " #field);
SALP_ROBOT_PHYS(SALP_ROBOT_PHYS_CHECK)
#undef SALP_ROBOT_PHYS_CHECK
static_assert((int)kRobotPhysCount == (int)SALP_RP_COUNT, "parameter rows");

// ------------------------------------------------------------------ host side: salp_robot_config_t -> RobotParams
// The reference's defaults (include/salp_robot.h): what salp_robot_config_default() hands out.
inline void robot_config_default(salp_robot_config_t* c) {
  memset(c, 0, sizeof(*c));
  c->struct_size = (uint32_t)sizeof(*c);
  c->width = 900; c->height = 700; c->tank_margin = 50.0;
  c->dry_mass = 1.0; c->init_length = 0.3; c->init_width = 0.15; c->max_contraction = 0.06; c->density = 1000.0;
  c->dt = 0.01; c->drag_coefficient_min = 0.4; c->drag_coefficient_max = 1.0;
  c->nozzle_length1 = c->nozzle_length2 = c->nozzle_length3 = 0.05;
  c->nozzle_area = 0.00016; c->nozzle_mass = 1.0; c->nozzle_gamma = kPi / 4; c->max_cycles = 500;
}

// What salp_robot_vec_create refuses before it touches a device.  SALP_OK, or SALP_ERR_INVALID with the reason in *why.
inline int check_robot_create(const salp_robot_config_t* cfg, int64_t n_envs, int64_t env_index_base, const char** why) {
  const auto refuse = [why](const char* msg) { *why = msg; return (int)SALP_ERR_INVALID; };
  if (!cfg || cfg->struct_size != sizeof(salp_robot_config_t)) return refuse("salp_robot_config_t.struct_size mismatch");
  if (n_envs <= 0 || env_index_base < 0) return refuse("n_envs / env_index_base out of range");
  if (!(cfg->dt > 0) || !(cfg->init_width > 0) || !(cfg->nozzle_area > 0)) return refuse("dt, init_width, nozzle_area must be positive");
  return (int)SALP_OK;
}

inline RobotParams make_robot_params(const salp_robot_config_t& cfg, int64_t n_envs, uint64_t seed, int64_t env_index_base) {
  RobotParams P = {};
#define SALP_ROBOT_PHYS_COPY(field, row, member) P.member = cfg.field;
  SALP_ROBOT_PHYS(SALP_ROBOT_PHYS_COPY)
#undef SALP_ROBOT_PHYS_COPY
  P.dt = cfg.dt;
  const double scale = 200.0;
  P.x_min = (-(double)cfg.width / 2 + cfg.tank_margin) / scale;
  P.x_span = ((double)cfg.width / 2 - cfg.tank_margin) / scale - P.x_min;
  P.y_min = (-(double)cfg.height / 2 + cfg.tank_margin) / scale;
  P.y_span = ((double)cfg.height / 2 - cfg.tank_margin) / scale - P.y_min;
  P.max_cycles = cfg.max_cycles;
  P.seed_lo = (uint32_t)seed; P.seed_hi = (uint32_t)(seed >> 32);
  P.env_base = (uint64_t)env_index_base; P.n = n_envs; P.pitch = (n_envs + 63) / 64 * 64;
  return P;
}

// Longest cycle a history may have to hold, in Euler steps: the step kernel's own count for a cycle of kMaxCycleTime
// (the same fp64 accumulation of dt).  -1 for a dt so small that this exceeds kMaxHistorySteps: the history and
// trajectory calls refuse such a handle rather than count (below ~1e-17 s the sum would never reach kMaxCycleTime).
inline int64_t robot_max_steps(double dt) {
  if (!(kMaxCycleTime / dt <= (double)kMaxHistorySteps)) return -1;
  double t = 0.0;
  int64_t k = 0;
  while (t < kMaxCycleTime && k <= kMaxHistorySteps) { t += dt; ++k; }
  return k > kMaxHistorySteps ? -1 : k;
}

// ceil(max_steps / stride) + 1 samples, or -1 (max_steps = robot_max_steps(dt), stride >= 1)
inline int64_t history_capacity(int64_t max_steps, int32_t stride) {
  return max_steps < 0 ? -1 : (max_steps + stride - 1) / stride + 1;
}

inline int refuse_robot_call(char* msg, size_t msg_size, const char* text) {
  snprintf(msg, msg_size, "%s", text);
  return (int)SALP_ERR_INVALID;
}

// What salp_robot_vec_step_history refuses once it has a handle (n envs, max_steps) and actions.  SALP_OK, or
// SALP_ERR_INVALID with the reason in msg.  *plain_step: the range is empty, the call is salp_robot_vec_step and
// nothing past the range was looked at.
inline int check_history_args(int64_t n, int64_t max_steps, int64_t hist_begin, int64_t hist_count, int32_t stride,
                              int32_t capacity, const void* history, uint32_t flags, bool* plain_step, char* msg,
                              size_t msg_size) {
  *plain_step = false;
  if (stride < 1) return refuse_robot_call(msg, msg_size, "history stride must be >= 1");
  if (hist_count < 0 || hist_begin < 0 || hist_begin > n || hist_count > n - hist_begin)
    return refuse_robot_call(msg, msg_size, "history env range [hist_begin, hist_begin + hist_count) is outside [0, n_envs)");
  if (hist_count == 0) { *plain_step = true; return (int)SALP_OK; }
  const int64_t need_cap = history_capacity(max_steps, stride);
  if (need_cap < 0)
    return refuse_robot_call(msg, msg_size, "dt is too small to record a history (more than 2^24 Euler steps per cycle)");
  if ((int64_t)capacity < need_cap) {
    snprintf(msg, msg_size, "history capacity %d is below salp_robot_vec_history_capacity = %lld", (int)capacity, (long long)need_cap);
    return (int)SALP_ERR_INVALID;
  }
  if (!history) return refuse_robot_call(msg, msg_size, "history is NULL while hist_count > 0");
  if ((flags & 1u) && ((uintptr_t)history % 16u) != 0)
    return refuse_robot_call(msg, msg_size, "device history must be 16-byte aligned");
  return (int)SALP_OK;
}

// What salp_robot_vec_trajectory refuses once it has a handle (max_steps) and actions.
inline int check_trajectory_args(int64_t max_steps, int32_t cycles, uint32_t flags, bool has_expected, bool has_metrics,
                                 char* msg, size_t msg_size) {
  if (cycles < 1 || cycles > SALP_ROBOT_MAX_TRAJECTORY_CYCLES) {
    snprintf(msg, msg_size, "cycles must be in [1, %d]", (int)SALP_ROBOT_MAX_TRAJECTORY_CYCLES);
    return (int)SALP_ERR_INVALID;
  }
  if (flags & ~(1u | (uint32_t)SALP_ROBOT_PER_ROBOT_ACTIONS)) return refuse_robot_call(msg, msg_size, "unknown flag bits");
  if (has_metrics && !has_expected) return refuse_robot_call(msg, msg_size, "metrics need expected states");
  // the same refusal as the history calls: with such a dt one cycle of the kMaxCycleTime cut exceeds 2^24 Euler steps
  if (max_steps < 0) return refuse_robot_call(msg, msg_size, "dt is too small (more than 2^24 Euler steps per cycle)");
  return (int)SALP_OK;
}

// The rollout kernel's service period M (salp_robot_kernels.h): a lane whose cycle has ended waits at most M Euler
// iterations of its wavefront for its next cycle; 0 = never, the synchronised form.  kRolloutPeriod is what the library
// runs (the measured choice); the others are compiled for profiles/robot_rollout_perf.py and selected
// with SALP_ROBOT_ROLLOUT_M at create.
constexpr int kRolloutPeriods[] = {0, 32, 128, 512};
constexpr int kRolloutPeriod = 128;

// What salp_robot_vec_rollout and salp_robot_vec_rollout_policy refuse once they have a handle (max_steps).
// has_source: act (or the policy) is not NULL; has_main_output: one of obs, reward, terminated, truncated is not NULL.
inline int check_rollout_args(int64_t max_steps, int32_t horizon, uint32_t flags, bool has_source, bool has_main_output,
                              char* msg, size_t msg_size) {
  if (!has_source) return refuse_robot_call(msg, msg_size, "act / policy is NULL");
  if (horizon < 1 || horizon > SALP_ROBOT_MAX_ROLLOUT_CYCLES) {
    snprintf(msg, msg_size, "horizon must be in [1, %d]", (int)SALP_ROBOT_MAX_ROLLOUT_CYCLES);
    return (int)SALP_ERR_INVALID;
  }
  if (flags & ~1u) return refuse_robot_call(msg, msg_size, "unknown flag bits");
  if (!has_main_output) return refuse_robot_call(msg, msg_size, "one of obs, reward, terminated, truncated is required");
  // the same refusal as the history and trajectory calls: the loop's iteration bound is counted in Euler steps
  if (max_steps < 0) return refuse_robot_call(msg, msg_size, "dt is too small (more than 2^24 Euler steps per cycle)");
  return (int)SALP_OK;
}

// What salp_robot_vec_evaluate_policy and salp_robot_vec_evaluate_policy_sampled refuse once they have a handle (max_steps)
// and a policy.  own_policy: the policy was created on this handle; sampled: the call is the sampled one; gaussian: the
// policy has a log-std head; device_ptrs is bit 0 of flags.
inline int check_evaluate_args(int64_t max_steps, int32_t horizon, uint32_t flags, const void* rec, bool own_policy, bool sampled,
                               bool gaussian, char* msg, size_t msg_size) {
  if (!rec) return refuse_robot_call(msg, msg_size, "rec is NULL");
  if (horizon < 1 || horizon > SALP_ROBOT_MAX_ROLLOUT_CYCLES) {
    snprintf(msg, msg_size, "horizon must be in [1, %d]", (int)SALP_ROBOT_MAX_ROLLOUT_CYCLES);
    return (int)SALP_ERR_INVALID;
  }
  if (flags & ~(1u | (uint32_t)SALP_ROBOT_EVAL_ACCUMULATE | (uint32_t)SALP_ROBOT_EVAL_FIRST_EPISODE))
    return refuse_robot_call(msg, msg_size, "unknown flag bits");
  if ((flags & 1u) && ((uintptr_t)rec % 16u) != 0) return refuse_robot_call(msg, msg_size, "device rec must be 16-byte aligned");
  if (!own_policy) return refuse_robot_call(msg, msg_size, "the policy belongs to another handle");
  if (sampled && !gaussian)
    return refuse_robot_call(msg, msg_size, "sampling needs a Gaussian policy (salp_robot_policy_create_gaussian)");
  // the same refusal as the history, trajectory and rollout calls: the loop's iteration bound is counted in Euler steps
  if (max_steps < 0) return refuse_robot_call(msg, msg_size, "dt is too small (more than 2^24 Euler steps per cycle)");
  return (int)SALP_OK;
}

// The iteration bound of the rollout kernel's loop.  A lane's cycle takes at most max_steps iterations, and the lane
// waits at most `period` iterations for the service point that ends it and opens the next one (period 0: the lanes of
// a wavefront go cycle by cycle, each round at most max_steps iterations and one service point); horizon cycles and
// the service point behind the last one, plus one iteration each for the rounds that run no Euler step.
inline int64_t rollout_max_iters(int32_t horizon, int64_t max_steps, int period) {
  return ((int64_t)horizon + 1) * (max_steps + (int64_t)period + 1);
}

// Bin of the cycle-length schedule for the Box action (a0, a1, .): the cycle's length as set_control will compute it,
// (contract + release) time of the contraction plus the coast, on a scale of kSchedBins over [0, kMaxCycleTime].
SALP_HOST_DEVICE inline int schedule_bin(float a0, float a1) {
  const double contraction = (double)a0 * kActContraction;
  const double total = contraction * (kContractTime / kActContraction + kReleaseTime / kActContraction) + (double)a1 * kActCoast;
  const double b = total * ((kSchedBins - 1) / kMaxCycleTime);
  if (!(b > 0.0)) return 0;                          // also NaN
  return b >= (double)(kSchedBins - 1) ? kSchedBins - 1 : (int)b;
}

}  // namespace
