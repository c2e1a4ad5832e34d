// salp_robot.hip — batched HEAD simulator for gfx950 and the C ABI of
// include/salp_robot.h: the reference's `Robot.step_through_cycle` (src/salp/environments/robot.py)
// under `SalpRobotEnv.step/reset` (src/salp/environments/salp_robot_env.py), one robot per lane.
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
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <stdlib.h>

#include <new>
#include <string>
#include <vector>

#include "../../include/salp_robot.h"
#include "salp_philox.h"   // philox4x32_10, u53
#include "salp_fp64_math.h"   // sincos_small, sincos_euler, advance_euler_sincos, rcp_nr, sqrt_nr
#include "salp_host.h"        // fail, HIP_TRY, DeviceScope, check_device_id, CallFrame, launch_1d, StageBuffer, staged()

using namespace salp;

namespace {

constexpr int kRBlock = 256;
constexpr double kPi = 3.141592653589793;

struct RobotParams {
  double dry_mass, init_length, init_width, max_contraction, density, dt, cd_min, cd_max;
  double nz_l1, nz_l2, nz_area, nz_mass, nz_gamma;
  double x_min, x_span, y_min, y_span;   // target placement, salp_robot_env.py:241-250
  int max_cycles;
  uint32_t seed_lo, seed_hi;
  uint64_t env_base;
  int64_t n, pitch;
};

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
// first) gives the order the step kernel walks the envs in; three small launches, no host round trip.
// Blocks of 1024 envs histogram in LDS first, so a block makes at most one global atomic per bin
// (one global atomic per env measured 45 us per pass at 262144 envs, 7 % of the step).
constexpr int kSchedBins = 256;
constexpr double kMaxCycleTime = 14.6;   // s; an in-Box action asks for at most 0.06 * (3 + 1.5) / 0.06 + 10 = 14.5 s
constexpr int kSchedBlock = 1024;

__device__ __forceinline__ int schedule_bin(const RobotParams& P, const float* act, int64_t i) {
  const double contraction = (double)act[i * 3 + 0] * 0.06;
  const double total = contraction * (3.0 / 0.06 + 1.5 / 0.06) + (double)act[i * 3 + 1] * 10.0;
  const double b = total * ((kSchedBins - 1) / 14.6);
  if (!(b > 0.0)) return 0;                          // also NaN
  return b >= (double)(kSchedBins - 1) ? kSchedBins - 1 : (int)b;
}
__global__ __launch_bounds__(kSchedBlock) void robot_schedule_count(RobotParams P, const float* act, uint32_t* bins) {
  __shared__ uint32_t hist[kSchedBins];
  const int t = threadIdx.x;
  if (t < kSchedBins) hist[t] = 0u;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kSchedBlock + t;
  if (i < P.n) atomicAdd(&hist[schedule_bin(P, act, i)], 1u);
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
  if (i < P.n) { b = schedule_bin(P, act, i); rank = atomicAdd(&hist[b], 1u); }
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
constexpr int32_t kMaxTrajectoryCycles = SALP_ROBOT_MAX_TRAJECTORY_CYCLES;

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
  // this robot's parameters: one coalesced load per row of the table.  Without a table every lane takes the config's
  // values and runs the same code, so that path is bit-identical to a table filled with them.
  RobotParams P = P0;
  if (J.params) {
    static_assert(SALP_RP_DRY_MASS == 0 && SALP_RP_INIT_LENGTH == 1 && SALP_RP_INIT_WIDTH == 2 && SALP_RP_MAX_CONTRACTION == 3 &&
                  SALP_RP_DENSITY == 4 && SALP_RP_DRAG_COEFFICIENT_MIN == 5 && SALP_RP_DRAG_COEFFICIENT_MAX == 6 &&
                  SALP_RP_NOZZLE_LENGTH1 == 7 && SALP_RP_NOZZLE_LENGTH2 == 8 && SALP_RP_NOZZLE_AREA == 9 &&
                  SALP_RP_NOZZLE_MASS == 10 && SALP_RP_NOZZLE_GAMMA == 11 && SALP_RP_COUNT == 12, "parameter rows");
    const double* q = J.params + i;
    P.dry_mass = q[0 * n]; P.init_length = q[1 * n]; P.init_width = q[2 * n]; P.max_contraction = q[3 * n];
    P.density = q[4 * n]; P.cd_min = q[5 * n]; P.cd_max = q[6 * n]; P.nz_l1 = q[7 * n]; P.nz_l2 = q[8 * n];
    P.nz_area = q[9 * n]; P.nz_mass = q[10 * n]; P.nz_gamma = q[11 * n];
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

// ---- host side (fail, HIP_TRY, CallFrame, launch_1d, staged(): salp_host.h) -------------------------------------------------
struct salp_robot_vec {
  salp_robot_config_t cfg;
  RobotParams P;
  RobotState S;
  int device;
  int64_t n;
  StageBuffer stage;  // staging for host-pointer calls (shrinks again after a large history, see StageBuffer)
  uint32_t* bins;     // [kSchedBins]
  int32_t* order;     // [n]
  bool schedule;      // walk the envs longest cycle first (see robot_schedule_*)
  int64_t max_steps;  // robot_max_steps(dt), counted at create
};

// Longest cycle a history may have to hold, in Euler steps: the step kernel's own count for a cycle of kMaxCycleTime
// (the same fp64 accumulation of dt).  -1 for a dt so small that this exceeds kMaxHistorySteps: the history and
// trajectory calls refuse such a handle rather than count (below ~1e-17 s the sum would never reach 14.6 s).
constexpr int64_t kMaxHistorySteps = (int64_t)1 << 24;
static int64_t robot_max_steps(double dt) {
  if (!(kMaxCycleTime / dt <= (double)kMaxHistorySteps)) return -1;
  double t = 0.0;
  int64_t k = 0;
  while (t < kMaxCycleTime && k <= kMaxHistorySteps) { t += dt; ++k; }
  return k > kMaxHistorySteps ? -1 : k;
}

// Below this many envs every wavefront has an execution unit to itself and the launch lasts as long as
// its slowest env whatever the order.  SALP_ROBOT_SCHEDULE=0/1 overrides (tests run both ways).
static const int64_t kScheduleMinEnvs = 32768;

static int launch_robot_step(salp_robot_vec* h, const float* act, float* obs, float* reward, uint8_t* terminated,
                             uint8_t* truncated, float* final_obs, int32_t* inner_steps, hipStream_t st,
                             const RobotHistory* hist = nullptr) {
  const int32_t* order = nullptr;
  if (h->schedule) {
    HIP_TRY(hipMemsetAsync(h->bins, 0, kSchedBins * sizeof(uint32_t), st));
    int rc = launch_1d(robot_schedule_count, h->n, kSchedBlock, st, h->P, act, h->bins);
    if (rc == SALP_OK) rc = launch_1d(robot_schedule_scan, kSchedBins, kSchedBins, st, h->bins);     // one workgroup
    if (rc == SALP_OK) rc = launch_1d(robot_schedule_scatter, h->n, kSchedBlock, st, h->P, act, h->bins, h->order);
    if (rc != SALP_OK) return rc;
    order = h->order;
  }
  if (hist && hist->count > 0)
    return launch_1d(salp_robot_step_record_kernel, h->n, kRBlock, st, h->P, h->S, act, obs, reward, terminated, truncated,
                     final_obs, inner_steps, order, *hist);
  return launch_1d(salp_robot_step_kernel, h->n, kRBlock, st, h->P, h->S, act, obs, reward, terminated, truncated, final_obs,
                   inner_steps, order);
}

extern "C" {

const char* salp_robot_last_error(void) { return g_err.c_str(); }

int salp_robot_config_default(salp_robot_config_t* c) {
  if (!c) return fail(SALP_ERR_INVALID, "cfg is NULL");
  memset(c, 0, sizeof(*c));
  c->struct_size = (uint32_t)sizeof(*c);
  c->width = 900; c->height = 700; c->tank_margin = 50.0;
  c->dry_mass = 1.0; c->init_length = 0.3; c->init_width = 0.15; c->max_contraction = 0.06; c->density = 1000.0;
  c->dt = 0.01; c->drag_coefficient_min = 0.4; c->drag_coefficient_max = 1.0;
  c->nozzle_length1 = c->nozzle_length2 = c->nozzle_length3 = 0.05;
  c->nozzle_area = 0.00016; c->nozzle_mass = 1.0; c->nozzle_gamma = kPi / 4; c->max_cycles = 500;
  return 0;
}

int salp_robot_vec_reset(salp_robot_vec_t* h, const uint8_t* mask, float* obs, uint32_t flags, void* stream);

int salp_robot_vec_create(const salp_robot_config_t* cfg, int64_t n_envs, int device_id, uint64_t seed,
                          int64_t env_index_base, salp_robot_vec_t** out) {
  if (!out) return fail(SALP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!cfg || cfg->struct_size != sizeof(salp_robot_config_t)) return fail(SALP_ERR_INVALID, "salp_robot_config_t.struct_size mismatch");
  if (n_envs <= 0 || env_index_base < 0) return fail(SALP_ERR_INVALID, "n_envs / env_index_base out of range");
  if (!(cfg->dt > 0) || !(cfg->init_width > 0) || !(cfg->nozzle_area > 0)) return fail(SALP_ERR_INVALID, "dt, init_width, nozzle_area must be positive");
  int rc = check_device_id(device_id);
  if (rc != SALP_OK) return rc;
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(device_id));
  salp_robot_vec* h = new (std::nothrow) salp_robot_vec();     // value-initialised: every field zero
  if (!h) return fail(SALP_ERR_OOM, "host allocation failed");
  h->cfg = *cfg; h->device = device_id; h->n = n_envs;
  h->stage.shrink = true;
  h->max_steps = robot_max_steps(cfg->dt);
  RobotParams& P = h->P;
  P.dry_mass = cfg->dry_mass; P.init_length = cfg->init_length; P.init_width = cfg->init_width;
  P.max_contraction = cfg->max_contraction; P.density = cfg->density; P.dt = cfg->dt;
  P.cd_min = cfg->drag_coefficient_min; P.cd_max = cfg->drag_coefficient_max;
  P.nz_l1 = cfg->nozzle_length1; P.nz_l2 = cfg->nozzle_length2; P.nz_area = cfg->nozzle_area;
  P.nz_mass = cfg->nozzle_mass; P.nz_gamma = cfg->nozzle_gamma;
  const double scale = 200.0;
  P.x_min = (-(double)cfg->width / 2 + cfg->tank_margin) / scale;
  P.x_span = ((double)cfg->width / 2 - cfg->tank_margin) / scale - P.x_min;
  P.y_min = (-(double)cfg->height / 2 + cfg->tank_margin) / scale;
  P.y_span = ((double)cfg->height / 2 - cfg->tank_margin) / scale - P.y_min;
  P.max_cycles = cfg->max_cycles;
  P.seed_lo = (uint32_t)seed; P.seed_hi = (uint32_t)(seed >> 32);
  P.env_base = (uint64_t)env_index_base; P.n = n_envs; P.pitch = (n_envs + 63) / 64 * 64;
  const size_t bytes = (size_t)SALP_R_COUNT * (size_t)P.pitch * sizeof(double);
  hipError_t e = hipMalloc((void**)&h->S.f, bytes);
  if (e == hipSuccess) e = hipMemset(h->S.f, 0, bytes);
  h->schedule = n_envs >= kScheduleMinEnvs;
  if (const char* ev = getenv("SALP_ROBOT_SCHEDULE")) h->schedule = ev[0] == '1';
  if (n_envs > INT32_MAX) h->schedule = false;
  if (e == hipSuccess && h->schedule) e = hipMalloc((void**)&h->bins, kSchedBins * sizeof(uint32_t));
  if (e == hipSuccess && h->schedule) e = hipMalloc((void**)&h->order, (size_t)n_envs * sizeof(int32_t));
  if (e != hipSuccess) { std::string m = std::string("state allocation: ") + hipGetErrorString(e); salp_robot_vec_destroy(h); return fail(SALP_ERR_OOM, m); }
  rc = salp_robot_vec_reset(h, nullptr, nullptr, 1u, nullptr);   // train_robot.py:16 angles (0, 0) are the zeroed rows
  if (rc == 0 && hipDeviceSynchronize() != hipSuccess) rc = fail(SALP_ERR_HIP, "initial reset failed");
  if (rc != 0) { std::string m = g_err; salp_robot_vec_destroy(h); g_err = m; return rc; }
  *out = h;
  return 0;
}

void salp_robot_vec_destroy(salp_robot_vec_t* h) {
  if (!h) return;
  DeviceScope dev_scope;
  (void)dev_scope.enter(h->device);
  if (h->S.f) (void)hipFree(h->S.f);
  if (h->bins) (void)hipFree(h->bins);
  if (h->order) (void)hipFree(h->order);
  delete h;     // the staging block goes with it
}

int64_t salp_robot_vec_num_envs(const salp_robot_vec_t* h) { return h ? h->n : 0; }

int salp_robot_vec_reset(salp_robot_vec_t* h, const uint8_t* mask, float* obs, uint32_t flags, void* stream) {
  if (!h) return fail(SALP_ERR_INVALID, "handle is NULL");
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  HostStream s[] = {stream_in(mask, (size_t)h->n), stream_out(obs, (size_t)h->n * 6)};
  return staged(h->stage, f.st, flags & 1u, s, [&] {
    return launch_1d(salp_robot_reset_kernel, h->n, kRBlock, f.st, h->P, h->S, s[0].as<const uint8_t>(), s[1].as<float>(), 1);
  });
}

// salp_robot_vec_step (H == NULL) and salp_robot_vec_step_history (H: the caller's range and pointers, count > 0);
// the arguments have been checked.
static int robot_step_impl(salp_robot_vec_t* h, const float* act, float* obs, float* reward, uint8_t* terminated,
                           uint8_t* truncated, float* final_obs, int32_t* inner_steps, const RobotHistory* H, uint32_t flags,
                           void* stream) {
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  hipStream_t st = f.st;
  // The two forms are kept apart here: with a history the host-pointer form is more than copies around the launch (a
  // scratch piece for the samples, a second copy once the lengths are known), which staged() does not take on.
  if (flags & 1u) return launch_robot_step(h, act, obs, reward, terminated, truncated, final_obs, inner_steps, st, H);
  // host pointers.  final_obs goes in as well as out: only the rows of ended episodes are written.  The history stays on
  // the device until the lengths are known (they are fetched even when the caller does not want them): it goes back as
  // `count` rows of the longest record of this call, one 2-D copy; nothing is copied in, so in rows with a shorter
  // record the samples past history_len are overwritten with unspecified values.
  const size_t n = (size_t)h->n, rows = H ? (size_t)H->count : 0;
  const size_t row = H ? (size_t)H->capacity * SALP_H_COUNT * sizeof(float) : 0;
  std::vector<int32_t> len(rows);
  HostStream s[] = {stream_in(act, n * 3), stream_out(obs, n * 6), stream_out(final_obs, n * 6, true), stream_out(reward, n),
                    stream_out(terminated, n), stream_out(truncated, n), stream_out(inner_steps, n),
                    stream_out(H ? len.data() : nullptr, rows), stream_scratch(rows * row)};
  const int rc = staged(h->stage, st, false, s, [&] {
    RobotHistory D;
    if (H) { D = *H; D.len = s[7].as<int32_t>(); D.hist = s[8].as<float>(); }
    return launch_robot_step(h, s[0].as<const float>(), s[1].as<float>(), s[3].as<float>(), s[4].as<uint8_t>(), s[5].as<uint8_t>(),
                             s[2].as<float>(), s[6].as<int32_t>(), st, H ? &D : nullptr);
  });
  if (rc != 0 || !H) return rc;
  int32_t longest = 0;
  for (int32_t v : len) longest = v > longest ? v : longest;
  HIP_TRY(hipMemcpy2DAsync(H->hist, row, s[8].dev, row, (size_t)longest * SALP_H_COUNT * sizeof(float), rows,
                           hipMemcpyDeviceToHost, st));
  if (H->len) memcpy(H->len, len.data(), rows * sizeof(int32_t));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

int salp_robot_vec_step(salp_robot_vec_t* h, const float* act, float* obs, float* reward, uint8_t* terminated,
                        uint8_t* truncated, float* final_obs, int32_t* inner_steps, uint32_t flags, void* stream) {
  if (!h || !act) return fail(SALP_ERR_INVALID, "handle / act is NULL");
  return robot_step_impl(h, act, obs, reward, terminated, truncated, final_obs, inner_steps, nullptr, flags, stream);
}

static int64_t history_capacity(const salp_robot_vec* h, int32_t stride) {   // ceil(T_max / stride) + 1 samples, or -1
  return h->max_steps < 0 ? -1 : (h->max_steps + stride - 1) / stride + 1;
}

int32_t salp_robot_vec_history_capacity(const salp_robot_vec_t* h, int32_t stride) {
  if (!h || stride < 1) return -1;
  return (int32_t)history_capacity(h, stride);
}

int salp_robot_vec_step_history(salp_robot_vec_t* h, const float* act, float* obs, float* reward, uint8_t* terminated,
                                uint8_t* truncated, float* final_obs, int32_t* inner_steps, int64_t hist_begin,
                                int64_t hist_count, int32_t stride, int32_t capacity, float* history,
                                int32_t* history_len, uint32_t flags, void* stream) {
  if (!h || !act) return fail(SALP_ERR_INVALID, "handle / act is NULL");
  if (stride < 1) return fail(SALP_ERR_INVALID, "history stride must be >= 1");
  if (hist_count < 0 || hist_begin < 0 || hist_begin > h->n || hist_count > h->n - hist_begin)
    return fail(SALP_ERR_INVALID, "history env range [hist_begin, hist_begin + hist_count) is outside [0, n_envs)");
  if (hist_count == 0)
    return robot_step_impl(h, act, obs, reward, terminated, truncated, final_obs, inner_steps, nullptr, flags, stream);
  const int64_t need_cap = history_capacity(h, stride);
  if (need_cap < 0) return fail(SALP_ERR_INVALID, "dt is too small to record a history (more than 2^24 Euler steps per cycle)");
  if ((int64_t)capacity < need_cap)
    return fail(SALP_ERR_INVALID, "history capacity " + std::to_string(capacity) + " is below salp_robot_vec_history_capacity = " +
                     std::to_string(need_cap));
  if (!history) return fail(SALP_ERR_INVALID, "history is NULL while hist_count > 0");
  if ((flags & 1u) && ((uintptr_t)history % 16u) != 0) return fail(SALP_ERR_INVALID, "device history must be 16-byte aligned");
  RobotHistory H;
  H.hist = history; H.len = history_len; H.begin = hist_begin; H.count = hist_count; H.stride = stride; H.capacity = capacity;
  return robot_step_impl(h, act, obs, reward, terminated, truncated, final_obs, inner_steps, &H, flags, stream);
}

int salp_robot_vec_trajectory(salp_robot_vec_t* h, const double* params, const double* actions, int32_t cycles,
                              const double* expected, double* states, double* metrics, int32_t* inner_steps,
                              uint32_t flags, void* stream) {
  if (!h || !actions) return fail(SALP_ERR_INVALID, "handle / actions is NULL");
  if (cycles < 1 || cycles > kMaxTrajectoryCycles)
    return fail(SALP_ERR_INVALID, "cycles must be in [1, " + std::to_string(kMaxTrajectoryCycles) + "]");
  if (flags & ~(1u | (uint32_t)SALP_ROBOT_PER_ROBOT_ACTIONS)) return fail(SALP_ERR_INVALID, "unknown flag bits");
  if (metrics && !expected) return fail(SALP_ERR_INVALID, "metrics need expected states");
  // the same refusal as the history calls: with such a dt one cycle of the 14.6 s cut exceeds 2^24 Euler steps
  if (h->max_steps < 0) return fail(SALP_ERR_INVALID, "dt is too small (more than 2^24 Euler steps per cycle)");
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  const bool per_robot = (flags & SALP_ROBOT_PER_ROBOT_ACTIONS) != 0;
  RobotTrajectory J;
  J.cycles = cycles; J.per_robot = per_robot ? 1 : 0;
  const size_t n = (size_t)h->n, T = (size_t)cycles;
  HostStream s[] = {stream_in(params, (size_t)SALP_RP_COUNT * n), stream_in(actions, T * (per_robot ? n : 1) * 3),
                    stream_in(expected, T * 6), stream_out(states, T * n * 6), stream_out(metrics, n * SALP_RM_COUNT),
                    stream_out(inner_steps, T * n)};
  return staged(h->stage, f.st, flags & 1u, s, [&] {
    J.params = s[0].as<const double>(); J.actions = s[1].as<const double>(); J.expected = s[2].as<const double>();
    J.states = s[3].as<double>(); J.metrics = s[4].as<double>(); J.inner_steps = s[5].as<int32_t>();
    return launch_1d(salp_robot_trajectory_kernel, h->n, kRBlock, f.st, h->P, J);
  });
}

int salp_robot_vec_get_state(salp_robot_vec_t* h, double* state, uint32_t flags, void* stream) {
  if (!h || !state) return fail(SALP_ERR_INVALID, "handle / state is NULL");
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  hipStream_t st = f.st;
  // rows are [pitch] on the device and [n] in the snapshot
  HIP_TRY(hipMemcpy2DAsync(state, (size_t)h->n * sizeof(double), h->S.f, (size_t)h->P.pitch * sizeof(double),
                            (size_t)h->n * sizeof(double), SALP_R_COUNT,
                            (flags & 1u) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  if (!(flags & 1u)) HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

// Test support (salp_fp64_math.h): one of the fp64 primitives over host arrays, staged like the other host-pointer calls.
int salp_robot_math_probe(int device_id, int function, const double* in, double* out, int64_t n, int32_t steps) {
  if (!in || !out) return fail(SALP_ERR_INVALID, "in / out is NULL");
  if (n < 1 || n > ((int64_t)1 << 24)) return fail(SALP_ERR_INVALID, "n must be in [1, 2^24]");
  size_t rows_in = 1, rows_out = 2;
  switch (function) {
    case SALP_MATH_SINCOS_SMALL: case SALP_MATH_SINCOS_EULER: break;
    case SALP_MATH_ROTATE: rows_in = 3; break;
    case SALP_MATH_CHAIN:
      if (steps < 0 || steps > 65536) return fail(SALP_ERR_INVALID, "steps must be in [0, 65536]");
      rows_in = 1 + (size_t)steps; rows_out = 3;
      break;
    case SALP_MATH_RCP_NR: case SALP_MATH_SQRT_NR: rows_out = 1; break;
    default: return fail(SALP_ERR_INVALID, "unknown function code");
  }
  if (rows_in * (size_t)n * sizeof(double) > ((size_t)1 << 31)) return fail(SALP_ERR_INVALID, "input larger than 2 GiB");
  const int rc = check_device_id(device_id);
  if (rc != SALP_OK) return rc;
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(device_id));
  StageBuffer stage;     // the call's own, released on return
  HostStream s[] = {stream_in(in, rows_in * (size_t)n), stream_out(out, rows_out * (size_t)n)};
  return staged(stage, nullptr, false, s, [&] {
    return launch_1d(salp_robot_math_probe_kernel, n, kRBlock, nullptr, function, s[0].as<const double>(), s[1].as<double>(), n, steps);
  });
}

}  // extern "C"
