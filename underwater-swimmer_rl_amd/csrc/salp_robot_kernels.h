// salp_robot_kernels.h — all device code of the robot library, included by salp_robot.hip alone, which launches it
// (RobotParams, the constants and schedule_bin are salp_robot_params.h): the robot in
// registers (Rb) with load / store / rest / reset / observe, the reset kernel, the three kernels of the cycle-length
// schedule, the history sample store, the two step kernels (salp_robot_step_body.h), the trajectory kernel, the
// multi-cycle rollout kernel and the math-probe kernel (a policy's relayout and noise-step kernels are salp_vec.hip's,
// reached through salp_policy_upload.h).  One breathing cycle itself is
// salp_robot_cycle_body.h, made of the pieces salp_robot_cycle_control.h / _consts.h / _start.h and
// salp_robot_euler_step.h, which the rollout kernel includes one by one.
//
// One env step is one whole breathing cycle: up to ~1450 explicit-Euler steps of dt = 0.01 s, each a
// rigid-body update with diagonal mass / inertia, quadratic + linear drag, a jet force during the
// release phase, Euler-angle kinematics and a body->world rotation.  Unlike the SalpSnakeEnv kernel
// this one has a real inner hot loop and almost no memory traffic (27 doubles of state in, 6 floats
// out per cycle): it is bound by the fp64 VALU rate, not by HBM.
//   * state lives in VGPRs for the whole cycle; lanes run different step counts (the cycle length is
//     action-dependent), so the loop runs until the slowest lane of the wavefront is done;
//   * the nozzle geometry (IK solve, three rotation matrices, jet direction, moment arm) is constant
//     over a cycle and is evaluated once per env step;
//   * the 3x3 matrices of the reference are diagonal (mass, inertia) or rotations about one axis, so
//     they are written out as the handful of scalar products they are;
//   * fp64 throughout, in the reference's operation order where that is defined (the reference's own
//     3x3 products go through BLAS, so parity is a tolerance: tests/test_gpu_robot.py).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "salp_robot_params.h"   // RobotParams, kPi, kMaxCycleTime, kSchedBins, the action scales and rates, schedule_bin
#include "salp_philox.h"         // philox4x32_10, u53
#include "salp_fp64_math.h"      // sincos_small, sincos_euler, advance_euler_sincos, rcp_nr, sqrt_nr
#include "salp_policy.h"         // policy_eval, policy_eval_sampled and the policy block's header words

namespace {

using namespace salp;

constexpr int kRBlock = 256;

struct RobotState {
  double* f;    // [SALP_R_COUNT][pitch] (the public snapshot layout is also the device layout)
};

struct Rb {   // one robot in registers
  double pos[3], vel[3], eul[3], om[3], vw[3], prevI[3];
  double target[2], prev_dist, volume, angle1, angle2, time;
  int cycle;
  uint32_t rng;
};

__device__ __forceinline__ double clipd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ double sq(double x) { return x * x; }

__device__ __forceinline__ void load_robot(Rb& r, const RobotState& S, const RobotParams& P, int64_t i) {
  const int64_t p = P.pitch;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.pos[k] = S.f[(SALP_R_POS + k) * p + i]; r.vel[k] = S.f[(SALP_R_VEL + k) * p + i];
    r.eul[k] = S.f[(SALP_R_EULER + k) * p + i]; r.om[k] = S.f[(SALP_R_OMEGA + k) * p + i];
    r.vw[k] = S.f[(SALP_R_VEL_WORLD + k) * p + i]; r.prevI[k] = S.f[(SALP_R_PREV_I + k) * p + i];
  }
  r.target[0] = S.f[SALP_R_TARGET * p + i]; r.target[1] = S.f[(SALP_R_TARGET + 1) * p + i];
  r.prev_dist = S.f[SALP_R_PREV_DIST * p + i]; r.volume = S.f[SALP_R_VOLUME * p + i];
  r.angle1 = S.f[SALP_R_ANGLE1 * p + i]; r.angle2 = S.f[SALP_R_ANGLE2 * p + i];
  r.time = S.f[SALP_R_TIME * p + i];
  r.cycle = (int)S.f[SALP_R_CYCLE * p + i]; r.rng = (uint32_t)S.f[SALP_R_RNG * p + i];
}
__device__ __forceinline__ void store_robot(const Rb& r, const RobotState& S, const RobotParams& P, int64_t i) {
  const int64_t p = P.pitch;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    S.f[(SALP_R_POS + k) * p + i] = r.pos[k]; S.f[(SALP_R_VEL + k) * p + i] = r.vel[k];
    S.f[(SALP_R_EULER + k) * p + i] = r.eul[k]; S.f[(SALP_R_OMEGA + k) * p + i] = r.om[k];
    S.f[(SALP_R_VEL_WORLD + k) * p + i] = r.vw[k]; S.f[(SALP_R_PREV_I + k) * p + i] = r.prevI[k];
  }
  S.f[SALP_R_TARGET * p + i] = r.target[0]; S.f[(SALP_R_TARGET + 1) * p + i] = r.target[1];
  S.f[SALP_R_PREV_DIST * p + i] = r.prev_dist; S.f[SALP_R_VOLUME * p + i] = r.volume;
  S.f[SALP_R_ANGLE1 * p + i] = r.angle1; S.f[SALP_R_ANGLE2 * p + i] = r.angle2;
  S.f[SALP_R_TIME * p + i] = r.time;
  S.f[SALP_R_CYCLE * p + i] = (double)r.cycle; S.f[SALP_R_RNG * p + i] = (double)r.rng;
}

// robot.py:737-759 / 534-551 helpers on (length, width)
__device__ __forceinline__ double water_volume(double length, double width) {
  return 4.0 / 3 * kPi * (length / 2) * sq(width / 2);
}
__device__ __forceinline__ void inertia_diag(const RobotParams& P, double mass, double length, double width, double arm_norm2, double* I) {
  const double In = P.nz_mass * arm_norm2;
  const double hw2 = sq(width / 2), hl2 = sq(length / 2);
  I[0] = 0.2 * mass * (hw2 + hw2);
  I[1] = 0.2 * mass * (hl2 + hw2) + In;
  I[2] = 0.2 * mass * (hw2 + hl2) + In;
}
// |r_nozzle + r_robot|: R_br @ (base + R_mb @ middle) = (-(l1 + l2), 0, 0) for any joint angles
// (R_mb turns about z, the links lie on z; robot.py:132-151, 567-575)
__device__ __forceinline__ double arm_x(const RobotParams& P, double length) { return -(P.nz_l1 + P.nz_l2) + -length / 2; }

// robot.py:287-312 Robot.reset: at rest at the origin, rest shape, cycle time 0
__device__ __forceinline__ void rest_robot(Rb& r, const RobotParams& P) {
#pragma unroll
  for (int k = 0; k < 3; ++k) { r.pos[k] = 0.0; r.vel[k] = 0.0; r.eul[k] = 0.0; r.om[k] = 0.0; r.vw[k] = 0.0; }
  r.time = 0.0; r.cycle = 0;
  const double length = P.init_length, width = P.init_width;
  r.volume = water_volume(length, width);
  const double mass = P.dry_mass + P.density * r.volume + P.nz_mass;
  inertia_diag(P, mass, length, width, sq(arm_x(P, length)), r.prevI);
}
// Robot.reset + salp_robot_env.py:98-128 (new target, prev_dist)
__device__ __forceinline__ void reset_robot(Rb& r, const RobotParams& P, uint64_t genv) {
  const U4 w = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), r.rng, 16u, P.seed_lo, P.seed_hi);
  r.rng += 1u;
  r.target[0] = P.x_min + P.x_span * u53(w.x, w.y);
  r.target[1] = P.y_min + P.y_span * u53(w.z, w.w);
  rest_robot(r, P);
  const double dx = r.pos[0] - r.target[0], dy = r.pos[1] - r.target[1];
  r.prev_dist = sqrt(dx * dx + dy * dy);
}

__device__ __forceinline__ void observe_robot(const Rb& r, float* o) {   // salp_robot_env.py:400-420
  o[0] = (float)(r.pos[0] - r.target[0]); o[1] = (float)(r.pos[1] - r.target[1]);
  o[2] = (float)r.vel[0]; o[3] = (float)r.vel[1]; o[4] = (float)r.eul[2]; o[5] = (float)r.om[2];
}

__global__ __launch_bounds__(kRBlock) void salp_robot_reset_kernel(RobotParams P, RobotState S, const uint8_t* mask, float* obs, int do_reset) {
  const int64_t i = (int64_t)blockIdx.x * kRBlock + threadIdx.x;
  if (i >= P.n) return;
  Rb r;
  load_robot(r, S, P, i);
  if (do_reset && (!mask || mask[i])) {
    reset_robot(r, P, P.env_base + (uint64_t)i);
    store_robot(r, S, P, i);
  }
  if (obs) {
    float o[6];
    observe_robot(r, o);
#pragma unroll
    for (int k = 0; k < 6; ++k) obs[i * 6 + k] = o[k];
  }
}


// ---- cycle-length schedule ----------------------------------------------------------------------------
// A cycle lasts (50 + 25) * contraction + coast seconds, anything from 0 to 14.5 s (0..1450 Euler steps)
// depending on the action, and a wavefront runs until its slowest lane is done: with envs in index order
// about half the lane-steps are idle.  A counting sort on the step count (256 bins of ~6 steps, longest
// first; schedule_bin, salp_robot_params.h) gives the order the step kernel walks the envs in; three small
// launches, no host round trip.
// Blocks of 1024 envs histogram in LDS first, so a block makes at most one global atomic per bin
// (one global atomic per env measured 45 us per pass at 262144 envs, 7 % of the step).
constexpr int kSchedBlock = 1024;

__global__ __launch_bounds__(kSchedBlock) void robot_schedule_count(RobotParams P, const float* act, uint32_t* bins) {
  __shared__ uint32_t hist[kSchedBins];
  const int t = threadIdx.x;
  if (t < kSchedBins) hist[t] = 0u;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kSchedBlock + t;
  if (i < P.n) atomicAdd(&hist[schedule_bin(act[i * 3 + 0], act[i * 3 + 1])], 1u);
  __syncthreads();
  if (t < kSchedBins && hist[t]) atomicAdd(&bins[t], hist[t]);
}
// bins[k] <- number of envs in bins above k (longest cycles get the first positions)
__global__ __launch_bounds__(kSchedBins) void robot_schedule_scan(uint32_t* bins) {
  __shared__ uint32_t part[kSchedBins];
  const int t = threadIdx.x;
  const int k = kSchedBins - 1 - t;                  // thread t owns bin k (descending order)
  const uint32_t c = bins[k];
  part[t] = c;
  __syncthreads();
  for (int d = 1; d < kSchedBins; d <<= 1) {
    const uint32_t v = t >= d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  bins[k] = part[t] - c;
}
__global__ __launch_bounds__(kSchedBlock) void robot_schedule_scatter(RobotParams P, const float* act, uint32_t* bins, int32_t* order) {
  __shared__ uint32_t hist[kSchedBins];              // count, then this block's base position, per bin
  const int t = threadIdx.x;
  if (t < kSchedBins) hist[t] = 0u;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kSchedBlock + t;
  int b = 0;
  uint32_t rank = 0;
  if (i < P.n) { b = schedule_bin(act[i * 3 + 0], act[i * 3 + 1]); rank = atomicAdd(&hist[b], 1u); }
  __syncthreads();
  if (t < kSchedBins && hist[t]) hist[t] = atomicAdd(&bins[t], hist[t]);
  __syncthreads();
  if (i < P.n) order[hist[b] + rank] = (int32_t)i;
}

// ---- per-Euler-step history (salp_robot_vec_step_history) ----------------------------------------------
// Recorded envs are the contiguous range [begin, begin + count); env i writes its samples to
// hist[(i - begin) * capacity * SALP_H_COUNT ...], one contiguous 64-byte sample per recorded step as four 16-byte
// stores.  The layout is env-major, so it does not depend on which lane the longest-cycle-first schedule put an env
// in.  Measured against a time-major layout [capacity][SALP_H_COUNT][count] and against non-temporal stores
// (profiles/robot_history_perf.py --layouts; the experiment builds -DSALP_ROBOT_HIST_TIME_MAJOR /
// -DSALP_ROBOT_HIST_NONTEMPORAL select those): plain stores let L2 merge each lane's four 16-byte pieces into one
// full 64-byte line before it goes to HBM, 4-5x the write rate of non-temporal ones, and beat time-major too.
struct RobotHistory {
  float* hist;          // [count][capacity][SALP_H_COUNT]
  int32_t* len;         // [count], nullable
  int64_t begin, count;
  int32_t stride, capacity;
};

typedef float f4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ void history_store(T v, T* p) {
#ifdef SALP_ROBOT_HIST_NONTEMPORAL
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

// Sample k of history row j, in the channel order of SALP_H_* (include/salp_robot.h)
__device__ __forceinline__ void store_history_sample(const RobotHistory& H, int64_t j, int32_t k, const Rb& r, double length,
                                                     double width, int state, float yaw) {
  static_assert(SALP_H_COUNT == 16 && SALP_H_POS == 0 && SALP_H_VEL == 3 && SALP_H_EULER == 6 && SALP_H_OMEGA == 9 &&
                SALP_H_LENGTH == 12 && SALP_H_WIDTH == 13 && SALP_H_STATE == 14 && SALP_H_NOZZLE_YAW == 15, "channel order");
  const f4 a = {(float)r.pos[0], (float)r.pos[1], (float)r.pos[2], (float)r.vel[0]};
  const f4 b = {(float)r.vel[1], (float)r.vel[2], (float)r.eul[0], (float)r.eul[1]};
  const f4 c = {(float)r.eul[2], (float)r.om[0], (float)r.om[1], (float)r.om[2]};
  const f4 d = {(float)length, (float)width, (float)state, yaw};
#ifdef SALP_ROBOT_HIST_TIME_MAJOR
  float* p = H.hist + (int64_t)k * SALP_H_COUNT * H.count + j;   // channel q of sample k at p[q * count]
  const int64_t n = H.count;
  history_store(a.x, p); p += n; history_store(a.y, p); p += n; history_store(a.z, p); p += n; history_store(a.w, p); p += n;
  history_store(b.x, p); p += n; history_store(b.y, p); p += n; history_store(b.z, p); p += n; history_store(b.w, p); p += n;
  history_store(c.x, p); p += n; history_store(c.y, p); p += n; history_store(c.z, p); p += n; history_store(c.w, p); p += n;
  history_store(d.x, p); p += n; history_store(d.y, p); p += n; history_store(d.z, p); p += n; history_store(d.w, p);
#else
  f4* p = reinterpret_cast<f4*>(H.hist + (j * H.capacity + k) * SALP_H_COUNT);
  history_store(a, p + 0);
  history_store(b, p + 1);
  history_store(c, p + 2);
  history_store(d, p + 3);
#endif
}

#ifndef SALP_ROBOT_WAVES
#define SALP_ROBOT_WAVES 2
#endif
// SalpRobotEnv.step (salp_robot_env.py:139-201): one breathing cycle per env (salp_robot_step_body.h)
__global__ __launch_bounds__(kRBlock) __attribute__((amdgpu_waves_per_eu(SALP_ROBOT_WAVES, SALP_ROBOT_WAVES)))
void salp_robot_step_kernel(RobotParams P, RobotState S, const float* act, float* obs,
                                                                  float* reward, uint8_t* terminated, uint8_t* truncated,
                                                                  float* final_obs, int32_t* inner_steps, const int32_t* order) {
  constexpr bool kRecord = false;
  const RobotHistory H = {};
#include "salp_robot_step_body.h"
}

// The same step, plus the cycle history of the envs [H.begin, H.begin + H.count)
__global__ __launch_bounds__(kRBlock) __attribute__((amdgpu_waves_per_eu(SALP_ROBOT_WAVES, SALP_ROBOT_WAVES)))
void salp_robot_step_record_kernel(RobotParams P, RobotState S, const float* act, float* obs, float* reward,
                                   uint8_t* terminated, uint8_t* truncated, float* final_obs, int32_t* inner_steps,
                                   const int32_t* order, RobotHistory H) {
  constexpr bool kRecord = true;
#include "salp_robot_step_body.h"
}

// ---- trajectory comparison (salp_robot_vec_trajectory) -------------------------------------------------
// compare_actions_with_states (compare_trajectories.py:19-117) for n robots, each with its own physical parameters:
// Robot.reset, then `cycles` breathing cycles, each reported as (x, y, vx, vy, yaw, yaw rate).  One robot per lane,
// in registers for the whole call; the handle's env state is neither read nor written.
struct RobotTrajectory {
  const double* params;     // [SALP_RP_COUNT][n], nullable: every robot takes the handle's config
  const double* actions;    // [cycles][3] (m, s, rad), or [cycles][n][3] with per_robot
  const double* expected;   // [cycles][6], nullable
  double* states;           // [cycles][n][6], nullable
  double* metrics;          // [n][SALP_RM_COUNT], nullable (only with expected)
  int32_t* inner_steps;     // [cycles][n], nullable
  int32_t cycles, per_robot;
};

__global__ __launch_bounds__(kRBlock) __attribute__((amdgpu_waves_per_eu(SALP_ROBOT_WAVES, SALP_ROBOT_WAVES)))
void salp_robot_trajectory_kernel(RobotParams P0, RobotTrajectory J) {
  constexpr bool kRecord = false;
  const RobotHistory H = {};
  const int64_t i0 = (int64_t)blockIdx.x * kRBlock + threadIdx.x;
  const bool active = i0 < P0.n;
  const int64_t i = active ? i0 : (P0.n - 1);
  const int64_t n = P0.n;
  // this robot's parameters: one coalesced load per row of the table (SALP_ROBOT_PHYS, salp_robot_params.h).  Without a
  // table every lane takes the config's values and runs the same code, so that path is bit-identical to a table filled
  // with them.
  RobotParams P = P0;
  if (J.params) {
    const double* q = J.params + i;
#define SALP_ROBOT_PHYS_LOAD(field, row, member) P.member = q[row * n];
    SALP_ROBOT_PHYS(SALP_ROBOT_PHYS_LOAD)
#undef SALP_ROBOT_PHYS_LOAD
  }
  Rb r;
  rest_robot(r, P);
  r.angle1 = 0.0; r.angle2 = 0.0;
  // compare_trajectories.py:77-86: sums in cycle order, kept in metrics[i] between cycles (not in registers: the
  // Euler loop needs them all); a NaN error makes the sums NaN and sticks in the max (like np.max; fmax drops it)
  double* m = (active && J.metrics) ? J.metrics + i * SALP_RM_COUNT : nullptr;
  for (int32_t t = 0; t < J.cycles; ++t) {
    const double* a = J.actions + (J.per_robot ? ((int64_t)t * n + i) * 3 : (int64_t)t * 3);
    const double contraction = a[0], coast_time = a[1], yaw = a[2];
#include "salp_robot_cycle_body.h"
    if (active) {
      const int64_t o = (int64_t)t * n + i;
      if (J.states) {   // time-major: the 64 lanes of a wavefront store 3 KB of contiguous bytes per cycle
        double* s = J.states + o * 6;
        s[0] = r.pos[0]; s[1] = r.pos[1]; s[2] = r.vel[0]; s[3] = r.vel[1]; s[4] = r.eul[2]; s[5] = r.om[2];
      }
      if (J.inner_steps) J.inner_steps[o] = steps;
      if (m) {
        const double* x = J.expected + (int64_t)t * 6;
        const double d0 = r.pos[0] - x[0], d1 = r.pos[1] - x[1], d2 = r.vel[0] - x[2], d3 = r.vel[1] - x[3];
        const double ep = sqrt(d0 * d0 + d1 * d1), ev = sqrt(d2 * d2 + d3 * d3);
        const double ea = fabs(r.eul[2] - x[4]), eo = fabs(r.om[2] - x[5]);
        if (t == 0) {
          m[0] = ep; m[1] = ev; m[2] = ea; m[3] = ep; m[4] = eo;
        } else {
          m[0] += ep; m[1] += ev; m[2] += ea; m[4] += eo;
          if (!(m[3] != m[3]) && !(ep <= m[3])) m[3] = ep;
        }
      }
    }
  }
  if (m) {
    const double c = (double)J.cycles;
    m[0] = m[0] / c; m[1] = m[1] / c; m[2] = m[2] / c; m[4] = m[4] / c;
  }
}

// ---- multi-cycle rollout (salp_robot_vec_rollout, salp_robot_vec_rollout_policy, _policy_sampled, _evaluate_policy) ------
// H env steps — H breathing cycles per robot — in one launch, env i on lane i, the robot in registers throughout; the
// actions are read (kActRead) or computed by the in-kernel MLP policy from the row the step before wrote (kActPolicy; or
// sampled from its Gaussian form, kActPolicySampled; salp_policy.h).  ONE loop over Euler iterations serves the whole launch.  Every lane carries its own step index
// t, its cycle (cycle_time, total and what the cycle pieces leave) and whether a cycle is in progress; a lane whose cycle
// is over and whose t is below H is DUE.  At a service point the due lanes, under EXEC masking, finish env step t
// (salp_robot_step_finish.h / _outputs.h: reward, flags, final_obs, autoreset, the stores of row t), advance t and, if
// t < H, take their next action and run the cycle's opening (salp_robot_cycle_control.h / _start.h).  A service point
// happens when no lane of the wavefront has an Euler step left, and on every M-th iteration on which some lane is due;
// M = 0 means never, which is the synchronised form: every lane waits for the slowest one of its wavefront, cycle by cycle,
// as a loop of salp_robot_step_kernel launches does.  With M > 0 a lane starts its next cycle at most M iterations after
// its own cycle ended, so a wavefront lasts about as long as its longest SUM of cycle lengths, not the sum of the longest
// cycles.  Service is batched because it is dear: the opening alone is several hundred fp64 instructions and a 64 x 64
// policy 4.7 k fmac, executed for however few lanes are due (DESIGN.md §8f-4 has the measured choice of M).
// Finished lanes (t == H) and padding lanes neither step nor wait.  The loop ends when no lane has t < H; it also carries the
// iteration bound rollout_max_iters (salp_robot_params.h), which no input can reach.  The state rows are written once, at the end.
struct RobotRollout {
  const float* act;        // kActRead: actions [H][n][3];  kActPolicy: the policy's device block (salp_policy.h)
  float* obs;              // [H][n][6]
  float* reward;           // [H][n]
  uint8_t* terminated;     // [H][n]
  uint8_t* truncated;      // [H][n]
  float* final_obs;        // [H][n][6], rows of finished envs only
  int32_t* inner_steps;    // [H][n]
  float* act_out;          // [H][n][3], kActPolicy / kActPolicySampled only           (every output nullable)
  int64_t max_iters;
  int32_t horizon;
  uint32_t eval_flags;     // kSigSummary only: SALP_ROBOT_EVAL_ACCUMULATE / _FIRST_EPISODE of the call's flags
  float* logp_out;         // [H][n], kActPolicySampled only
  int32_t* rec;            // kSigSummary only: [n][SALP_REVAL_WORDS], 16-byte aligned
};
// kActPolicySampled (salp_robot_vec_rollout_policy_sampled, include/salp_robot_sampled.h): the closed loop with the
// stochastic form of a Gaussian policy.  The policy's noise step n0 is read once at entry (wave-uniform); a lane served
// for its own env step t draws the Philox blocks (genv, n0 + t, 3) and (genv, n0 + t, 4) — a function of (env, t) alone,
// whichever iteration the lane is served on — and stores the sampled action and its log-probability for step t.
enum { kActRead = 0, kActPolicy = 1, kActPolicySampled = 2 };
enum { kRobotNoiseStream = 3 };     // fourth counter word of component 0 / 1's block; component 2's is one above
enum { ROBOT_POLICY_OBS = 6, ROBOT_POLICY_ACT = 3 };     // the policy's shape: salp_policy.h with 6 inputs and 3 components
// The output signature, SIG.  kSigSteps: the per-step blocks above.  kSigSummary (salp_robot_vec_evaluate_policy, _sampled;
// include/salp_robot_evaluate.h): no per-step output, one record of SALP_REVAL_WORDS words per robot in J.rec.  The loop,
// the service points, the cycle pieces and the policy evaluation are the same text, so a summary launch computes the
// bits of the per-step launch it stands for.  At a service point a due lane folds (float)rew, term, trunc and steps of
// its step into its record, which lives in J.rec between service points and not in registers (the Euler loop needs them
// all; a service point comes once per hundreds of Euler iterations, so 48 bytes read and written there cost nothing):
// the record is initialised at entry — zeroed, or with SALP_ROBOT_EVAL_ACCUMULATE left as the caller passed it.  With
// SALP_ROBOT_EVAL_FIRST_EPISODE a lane whose record has FIRST_END != 0, at entry or after its fold, is finished (t = H):
// it neither steps nor waits, like every finished lane.  Records of padding lanes and of rows >= n are never touched.
enum { kSigSteps = 0, kSigSummary = 1 };
typedef int32_t i4 __attribute__((ext_vector_type(4)));
static_assert(SALP_REVAL_WORDS == 12 && SALP_REVAL_RETURN == 0 && SALP_REVAL_FIRST_RETURN == 2 && SALP_REVAL_EULER_STEPS == 4 &&
              SALP_REVAL_FIRST_LENGTH == 6 && SALP_REVAL_FIRST_END == 7 && SALP_REVAL_EPISODES == 8 && SALP_REVAL_REACHED == 9 &&
              SALP_REVAL_FIRST_EULER_STEPS == 10, "the record is three 16-byte pieces: words 0-3, 4-7, 8-11");

__device__ __forceinline__ double words_as_double(int32_t lo, int32_t hi) {
  return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}

// One env step folded into the record at q (include/salp_robot_evaluate.h): three 16-byte loads, three 16-byte stores.
// Returns FIRST_END after the fold.
__device__ __forceinline__ int32_t fold_robot_record(i4* q, float rew, bool term, bool trunc, int steps) {
  i4 a = q[0], b = q[1], c = q[2];
  const double r = (double)rew;
  const uint64_t ret = (uint64_t)__double_as_longlong(words_as_double(a.x, a.y) + r);
  a.x = (int32_t)(uint32_t)ret; a.y = (int32_t)(uint32_t)(ret >> 32);
  const uint64_t euler = (((uint64_t)(uint32_t)b.y << 32) | (uint32_t)b.x) + (uint64_t)(int64_t)steps;
  b.x = (int32_t)(uint32_t)euler; b.y = (int32_t)(uint32_t)(euler >> 32);
  if (b.w == 0) {     // the first episode is still open: FIRST_RETURN, FIRST_LENGTH, FIRST_EULER_STEPS, FIRST_END
    const uint64_t first = (uint64_t)__double_as_longlong(words_as_double(a.z, a.w) + r);
    a.z = (int32_t)(uint32_t)first; a.w = (int32_t)(uint32_t)(first >> 32);
    b.z += 1;
    c.z += steps;
    b.w = term ? 1 : (trunc ? 2 : 0);     // terminated wins
  }
  c.x += (term || trunc) ? 1 : 0;
  c.y += term ? 1 : 0;
  q[0] = a; q[1] = b; q[2] = c;
  return b.w;
}

// what the opening of a cycle leaves for the Euler steps of that cycle (the names of the cycle pieces)
struct RobotCycle {
  double dir[3], contraction, refill_time, t_jet_end, t_coast_end, total, cycle_time;
  double mass, inv_m, kd, ktc, ax, I0, I1, I2, iI0, iI1, iI2, sp, cp, st, ct, ss, cs;
  int steps;
  bool settled;
};

// a value that is the same in every lane, in scalar registers
__device__ __forceinline__ double wave_uniform(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

template <int ACT, int M, int SIG = kSigSteps>
__global__ __launch_bounds__(kRBlock) __attribute__((amdgpu_waves_per_eu(SALP_ROBOT_WAVES, SALP_ROBOT_WAVES)))
void salp_robot_rollout_kernel(RobotParams P, RobotState S, RobotRollout J) {
  static_assert(M >= 0 && (M & (M - 1)) == 0, "M is 0 (never) or a power of two");
  static_assert(SIG == kSigSteps || (SIG == kSigSummary && ACT != kActRead), "a summary is of a closed loop");
  constexpr bool kRecord = false;
  const RobotHistory H = {};
  const int64_t i0 = (int64_t)blockIdx.x * kRBlock + threadIdx.x;
  const bool active = i0 < P.n;
  const int64_t i = active ? i0 : (P.n - 1);
  const uint64_t genv = P.env_base + (uint64_t)i;
  const int64_t n = P.n;
  const int32_t horizon = J.horizon;
  Rb r;
  load_robot(r, S, P, i);
  [[maybe_unused]] uint32_t pol_off = 0;      // a wavefront never mixes policies: its envs lie in one group of PH_GROUP envs
  if constexpr (ACT == kActPolicy || ACT == kActPolicySampled) {
    const int32_t* hd = reinterpret_cast<const int32_t*>(J.act);
    pol_off = (uint32_t)(i / (int64_t)hd[PH_GROUP]) * (uint32_t)hd[PH_STRIDE];
  }
  [[maybe_unused]] uint32_t noise0 = 0u;      // kActPolicySampled: low word of the policy's noise step at entry (wave-uniform)
  if constexpr (ACT == kActPolicySampled) {
    // the two PH_NOISE words, scalar loads through the constant address space like the weights (salp_policy.h); only the
    // low word enters the draw: n is the low 32 bits of n0 + t, and t < 2^31
    pol_int* hd = policy_block_header(J.act);
    const uint64_t n0 = ((uint64_t)(uint32_t)hd[PH_NOISE + 1] << 32) | (uint32_t)hd[PH_NOISE];
    noise0 = (uint32_t)n0;
  }

  // The lane's cycle, under the names salp_robot_euler_step.h reads; no cycle yet: nothing to step (cycle_time == total)
  const double contract_rate = kContractRate, release_rate = kReleaseRate;
  // The constants of the physical parameters are the same in every lane (P is the kernel argument): they are moved to
  // scalar registers, where they cost no VGPR across the service code (as VGPRs they were spilled to scratch and read
  // back inside the Euler step).
  double uni[4];
  {
#include "salp_robot_cycle_consts.h"
    uni[0] = dt; uni[1] = inv_dt; uni[2] = min_aspect; uni[3] = inv_aspect_span;
  }
  const double dt = wave_uniform(uni[0]), inv_dt = wave_uniform(uni[1]), min_aspect = wave_uniform(uni[2]),
               inv_aspect_span = wave_uniform(uni[3]);
  double dir[3] = {0.0, 0.0, 0.0};
  double contraction = 0.0, refill_time = 0.0, t_jet_end = 0.0, t_coast_end = 0.0, total = 0.0, cycle_time = 0.0;
  double mass = 0, inv_m = 0, kd = 0, ktc = 0, ax = 0, I0 = 0, I1 = 0, I2 = 0, iI0 = 0, iI1 = 0, iI2 = 0;
  double sp = 0, cp = 1, st = 0, ct = 1, ss = 0, cs = 1;
  int steps = 0;
  bool settled = false;
  // (named by the recording branch of the Euler step, which kRecord = false discards)
  [[maybe_unused]] const bool rec = false;
  [[maybe_unused]] const int64_t hj = 0;
  [[maybe_unused]] int32_t n_samples = 0, until_sample = 0;
  [[maybe_unused]] const float yaw_f = 0.f;

  int32_t t = active ? 0 : horizon;     // padding lanes are finished from the start
  bool running = false;                 // a cycle has been opened for env step t and that step is not finished yet
  if constexpr (SIG == kSigSummary) {
    if (active) {
      i4* const q = reinterpret_cast<i4*>(J.rec + i * SALP_REVAL_WORDS);
      if (!(J.eval_flags & (uint32_t)SALP_ROBOT_EVAL_ACCUMULATE)) {
        const i4 zero = {0, 0, 0, 0};
        q[0] = zero; q[1] = zero; q[2] = zero;
      } else if ((J.eval_flags & (uint32_t)SALP_ROBOT_EVAL_FIRST_EPISODE) && J.rec[i * SALP_REVAL_WORDS + SALP_REVAL_FIRST_END] != 0) {
        t = horizon;                    // its first episode ended in an earlier call: nothing to run
      }
    }
  }
  // One round per service point: the service code, then Euler iterations up to the next service point.  The Euler
  // iterations form an inner loop of their own so that the register allocator ranks what they read above what only the
  // service code reads (as one flat loop it reloaded two of the Euler step's operands from scratch on every iteration).
  int64_t iter = 0;
#pragma unroll 1
  for (;;) {
    {
      const bool due = !(cycle_time < total) && t < horizon;
      if (!__any(t < horizon)) break;
      if (due) {
        if (running) {     // env step t is over: due lanes are active lanes
          const int64_t row = (int64_t)t * n;
          float* const final_obs = (SIG == kSigSteps && J.final_obs) ? J.final_obs + row * 6 : nullptr;
#include "salp_robot_step_finish.h"
          ++t;
          if constexpr (SIG == kSigSummary) {
            const int32_t first_end = fold_robot_record(reinterpret_cast<i4*>(J.rec + i * SALP_REVAL_WORDS), (float)rew, term, trunc, steps);
            if ((J.eval_flags & (uint32_t)SALP_ROBOT_EVAL_FIRST_EPISODE) && first_end != 0) t = horizon;
          } else {
            float* const obs = J.obs ? J.obs + row * 6 : nullptr;
            float* const reward = J.reward ? J.reward + row : nullptr;
            uint8_t* const terminated = J.terminated ? J.terminated + row : nullptr;
            uint8_t* const truncated = J.truncated ? J.truncated + row : nullptr;
            int32_t* const inner_steps = J.inner_steps ? J.inner_steps + row : nullptr;
#include "salp_robot_step_outputs.h"
          }
          running = false;
        }
        if (t < horizon) {
          // the action of step t: of the row just written (the entry observation for t = 0), or read
          float a[3];
          if constexpr (ACT == kActPolicy || ACT == kActPolicySampled) {
            float x[6];
            observe_robot(r, x);
            [[maybe_unused]] float lp;
            if constexpr (ACT == kActPolicySampled) {
              // the draws of (env, step t): components 0 and 1 from the block of stream word 3, component 2 from the first
              // two words of the block of stream word 4 (include/salp_robot_sampled.h); the env's own counter is not consumed
              const uint32_t nt = noise0 + (uint32_t)t;
              const U4 w0 = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), nt, (uint32_t)kRobotNoiseStream, P.seed_lo, P.seed_hi);
              const U4 w1 = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), nt, (uint32_t)kRobotNoiseStream + 1u, P.seed_lo, P.seed_hi);
              const float z[3] = {policy_normal(w0.x, w0.y), policy_normal(w0.z, w0.w), policy_normal(w1.x, w1.y)};
              policy_eval_sampled<ROBOT_POLICY_OBS, ROBOT_POLICY_ACT>(J.act, pol_off, x, z, a, lp);
            } else {
              policy_eval<ROBOT_POLICY_OBS, ROBOT_POLICY_ACT>(J.act, pol_off, x, a);
            }
            if (SIG == kSigSteps && J.act_out) {
              float* ao = J.act_out + ((int64_t)t * n + i) * 3;
              ao[0] = a[0]; ao[1] = a[1]; ao[2] = a[2];
            }
            if constexpr (ACT == kActPolicySampled) {
              if (SIG == kSigSteps && J.logp_out) J.logp_out[(int64_t)t * n + i] = lp;
            }
          } else {
            const float* ai = J.act + ((int64_t)t * n + i) * 3;
            a[0] = ai[0]; a[1] = ai[1]; a[2] = ai[2];
          }
          RobotCycle c;
          {
            // _rescale_action (:129-137) in fp64, as in salp_robot_step_body.h
            const double contraction = (double)a[0] * kActContraction;
            const double coast_time = (double)a[1] * kActCoast;
            const double yaw = (double)a[2] * kActYaw;
#include "salp_robot_cycle_control.h"
#include "salp_robot_cycle_start.h"
            c = {{dir[0], dir[1], dir[2]}, contraction, refill_time, t_jet_end, t_coast_end, total, cycle_time,
                 mass, inv_m, kd, ktc, ax, I0, I1, I2, iI0, iI1, iI2, sp, cp, st, ct, ss, cs, steps, settled};
          }
          dir[0] = c.dir[0]; dir[1] = c.dir[1]; dir[2] = c.dir[2];
          contraction = c.contraction; refill_time = c.refill_time; t_jet_end = c.t_jet_end; t_coast_end = c.t_coast_end;
          total = c.total; cycle_time = c.cycle_time;
          mass = c.mass; inv_m = c.inv_m; kd = c.kd; ktc = c.ktc; ax = c.ax; I0 = c.I0; I1 = c.I1; I2 = c.I2;
          iI0 = c.iI0; iI1 = c.iI1; iI2 = c.iI2; sp = c.sp; cp = c.cp; st = c.st; ct = c.ct; ss = c.ss; cs = c.cs;
          steps = c.steps; settled = c.settled;
          running = true;
        }
      }
    }
    bool service;
#pragma unroll 1
    do {
      if (cycle_time < total) {
#include "salp_robot_euler_step.h"
      }
      ++iter;
      service = !__any(cycle_time < total);
      if constexpr (M > 0) service = service || ((iter & (int64_t)(M - 1)) == 0 && __any(!(cycle_time < total) && t < horizon));
    } while (!service && iter < J.max_iters);
    if (iter >= J.max_iters) break;
  }
  if (active) store_robot(r, S, P, i);
}

// ---- test support: the fp64 primitives on their own (salp_robot_math_probe, declared in salp_fp64_math.h) ----------
// Element i on thread i, so wavefront w holds the elements [64 w, 64 w + 64); `function` is uniform, so every vote
// inside is taken over the whole wavefront (over its lanes below n in the last one).
__global__ __launch_bounds__(kRBlock) void salp_robot_math_probe_kernel(int function, const double* in, double* out, int64_t n,
                                                                        int32_t steps) {
  const int64_t i = (int64_t)blockIdx.x * kRBlock + threadIdx.x;
  if (i >= n) return;
  switch (function) {
    case SALP_MATH_SINCOS_SMALL: { double s, c; sincos_small(in[i], s, c); out[i] = s; out[n + i] = c; break; }
    case SALP_MATH_SINCOS_EULER: { double s, c; sincos_euler(in[i], s, c); out[i] = s; out[n + i] = c; break; }
    case SALP_MATH_ROTATE: {
      double s = in[i], c = in[n + i];
      rotate_sincos(s, c, in[2 * n + i]);
      out[i] = s; out[n + i] = c;
      break;
    }
    case SALP_MATH_CHAIN: {
      double e = in[i], s, c, s1 = 0.0, c1 = 1.0, s2 = 0.0, c2 = 1.0;
      sincos_euler(e, s, c);
#pragma unroll 1
      for (int32_t k = 0; k < steps; ++k) {
        const double d = in[(int64_t)(1 + k) * n + i];
        e += d;
        advance_euler_sincos(e, 0.0, 0.0, d, 0.0, 0.0, s, c, s1, c1, s2, c2);
      }
      out[i] = s; out[n + i] = c; out[2 * n + i] = e;
      break;
    }
    case SALP_MATH_RCP_NR: out[i] = rcp_nr(in[i]); break;
    case SALP_MATH_SQRT_NR: out[i] = sqrt_nr(in[i]); break;
    default: break;
  }
}

}  // namespace
