// salp_params.h — the parameters of a snake-simulator launch: the packed breathing word, the launch-parameter block
// DevParams with its literal twin StdConsts and CV(), the SoA state layout and the statistics slots; and the host functions
// that derive a DevParams from a salp_config_t (default_config, validate, make_params, is_std) and check a host snapshot
// (check_snapshot).
//
// The header compiles in two ways, like salp_fp64_math.h:
//   * with hipcc: what the kernels and salp_vec.hip include, through salp_device.h;
//   * as plain host C++ (tests/params_host.cpp): everything but open_consts(), with the __host__ / __device__ qualifiers
//     and the constant address space dropped, so that the derivation of the constants is under test without a GPU.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SALP_HOST_DEVICE __host__ __device__
#else
#define SALP_HOST_DEVICE
#endif
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/salp_vec.h"   // salp_config_t, SALP_OK, SALP_ERR_INVALID, SALP_MAX_*, SALP_F_* / SALP_I_*

namespace salp {

// ---- packed breathing word: phase[1:0] | timer[9:2] | exhale_dur[17:10] | shape_hold[20:18]
SALP_HOST_DEVICE inline uint32_t pack_breath(int phase, int timer, int dur, int hold) {
  return (uint32_t)(phase & 3) | ((uint32_t)(timer & 255) << 2) | ((uint32_t)(dur & 255) << 10) |
         ((uint32_t)(hold & 7) << 18);
}
SALP_HOST_DEVICE inline int bw_phase(uint32_t w) { return (int)(w & 3u); }
SALP_HOST_DEVICE inline int bw_timer(uint32_t w) { return (int)((w >> 2) & 255u); }
SALP_HOST_DEVICE inline int bw_dur(uint32_t w) { return (int)((w >> 10) & 255u); }
SALP_HOST_DEVICE inline int bw_hold(uint32_t w) { return (int)((w >> 18) & 7u); }

// The key words of the draw streams are read through the constant address space: scalar loads (s_load_dwordx2, scalar
// cache) wherever a kernel draws, no vector-memory wait.  They only change between launches (salp_vec_reseed), and the
// scalar cache is invalidated at every kernel start.
#if defined(__HIPCC__)
typedef const uint32_t __attribute__((address_space(4))) seed_word_t;
#else
typedef const uint32_t seed_word_t;
#endif

// Constants derived on the host in fp64 exactly as the reference derives them.
struct DevParams;
#if defined(__HIPCC__)
typedef const DevParams __attribute__((address_space(4))) dev_params_c;   // the handle's copy in device memory, read with scalar loads
#else
typedef const DevParams dev_params_c;
#endif
struct DevParams {
  // geometry / legacy constants
  double W, H, half_W, half_H;
  double margin;            // tank_margin (50)
  double wall_hi_x, wall_hi_y;  // width - margin, height - margin (snake:226,228)
  double R;                 // base_radius
  double a_rest, b_rest;    // R*1.3, R*0.8             (legacy:190-191)
  double ab_full;           // R*1.1                    (legacy:209-210)
  double da_inh, db_inh;    // (end - start) inhaling   (legacy:212-213)
  double da_exh, db_exh;    // (end - start) exhaling   (legacy:245-246)
  double max_nozzle, nozzle_rate, thrust_force, drag, ang_drag;
  double exhale_dur_d;      // (double)exhale_duration
  double food_radius, min_food_dist2;   // 15, 80^2
  double food_xlo, food_xspan, food_ylo, food_yspan;  // random.uniform(lo, hi) = lo + span*u
  double food_reward, collision_penalty, time_penalty, efficiency_bonus, prox_w;
  // fp32 reciprocals for the observation
  double inv_W, inv_H, inv_pi, inv_R, inv_max_nozzle;
  float inv_diag;           // 1/sqrt(W^2+H^2)
  float tie_c0;             // constant term of the fp32 food keys' error bound, 1.4e-7 max(W, H)^2 (salp_food_reg.h)
  int inhale_dur, exhale_dur, cycle_len, max_steps_wo_food;
  int F, K;                 // food slots (num_food_items at creation), max_observed_food
  int F_base;               // base_num_food_items: foods of the next episodes, 0..F (snake:36, :144-148)
  int forced, random_food_count, respawn;
  int autoreset;            // 0: finished envs keep running (salp_config_t.no_autoreset)
  seed_word_t* seed;        // the two key words of the draw streams, in DEVICE memory (the handle's ColdBlock): a kernel
                            // reads them where it draws, so salp_vec_reseed() changes them without changing any launch
                            // parameter — a hipGraph captured before a reseed replays with the new key
  dev_params_c* self;       // this block in DEVICE memory (the handle's ColdBlock): where the STD = false kernels read their
                            // constants, function by function (open_consts below); always valid
  int use_mem;              // 1: read the constants through `self` (set by the kernel on its own copy, a compile-time constant
                            // there; 0 from the host)
  uint64_t env_base;        // global index of local env 0
  int64_t n;                // envs in this handle
  int64_t pitch;            // row pitch (elements) of the SoA state blocks
};

// Compile-time image of the reference's hard-coded constants (legacy:32-53, snake:53-54, 800x600).
// Kernels instantiated with STD = true read these literals (rematerialisable scalar immediates: no
// SGPR pressure, no spills); any other configuration takes the values from DevParams.
// The list is the one place that names them: X(type, name, literal) makes a member of StdConsts and a comparison of
// is_std() out of each line, so a constant that CV() can read is a constant that is_std() tests, and a name that
// DevParams lacks does not compile.
#define SALP_STD_CONSTS(X) \
  X(double, W, 800.0) X(double, H, 600.0) X(double, half_W, 400.0) X(double, half_H, 300.0) \
  X(double, margin, 50.0) X(double, wall_hi_x, 750.0) X(double, wall_hi_y, 550.0) \
  X(double, R, 30.0) X(double, a_rest, 39.0) X(double, b_rest, 24.0) X(double, ab_full, 33.0) \
  X(double, da_inh, -6.0) X(double, db_inh, 9.0) X(double, da_exh, 6.0) X(double, db_exh, -9.0) \
  X(double, max_nozzle, 1.0471975511965976) X(double, nozzle_rate, 0.05) X(double, thrust_force, 100.0) \
  X(double, drag, 0.98) X(double, ang_drag, 0.95) X(double, exhale_dur_d, 150.0) \
  X(double, food_radius, 15.0) X(double, min_food_dist2, 6400.0) \
  X(double, food_xlo, 65.0) X(double, food_xspan, 670.0) X(double, food_ylo, 65.0) X(double, food_yspan, 470.0) \
  X(double, inv_W, 1.0 / 800.0) X(double, inv_H, 1.0 / 600.0) X(double, inv_pi, 1.0 / 3.141592653589793) \
  X(double, inv_R, 1.0 / 30.0) X(double, inv_max_nozzle, 1.0 / 1.0471975511965976) \
  X(float, inv_diag, 1.0e-3f) \
  X(float, tie_c0, 0.0896f) \
  X(int, inhale_dur, 120) X(int, exhale_dur, 150) X(int, cycle_len, 330)
struct StdConsts {
#define SALP_STD_MEMBER(type, name, literal) static constexpr type name = literal;
  SALP_STD_CONSTS(SALP_STD_MEMBER)
#undef SALP_STD_MEMBER
};
// CV(name): the constant `name` for this instantiation.  STD = false: ~50 doubles that differ from the literals.  Taken from
// the by-value launch parameter they are all loop-invariant scalars: the compiler loads them once, needs ~100 SGPRs for
// them and spills ~90-115 of those to VGPR lanes, so that nearly every use in the step loop costs a v_readlane (the 8- and
// 12-slot kernels ran 17-25 % behind their literal-constant forms, profiles/r03/ab_notes.md session 15).  Instead every
// function that uses constants opens the handle's device copy through a pointer made opaque there (SALP_CONSTS): the scalar
// loads (s_load_dwordx2..x16, scalar cache) stay in that function, and the registers are free again after it.
// Measured (ab_pc_f*.json): 4- and 8-slot kernels -5 ... -15 % (125 VGPRs, four wavefronts per SIMD again); one-food +1.4 %,
// 12- and 16-slot kernels +13 % (two / three wavefronts per SIMD do not hide the scalar-load waits) — so a kernel chooses:
// it hands its functions a parameter block whose `use_mem` is a compile-time 0 to keep the by-value constants.
#if defined(__HIPCC__)
template <bool STD>
__device__ __forceinline__ dev_params_c* open_consts(const DevParams& P) {
  if constexpr (STD) return nullptr;
  else {
    // `use_mem` is a literal in the kernel's own copy of the parameters and every caller is __forceinline__: the test folds.
    // (Should it ever not fold, it is a wave-uniform run-time test and both forms stay correct: `self` is always valid.)
    if (!P.use_mem) return nullptr;
    // (the rare paths hand in the memory copy itself: its `self` word may arrive through a vector load)
    const uint64_t a = (uint64_t)(uintptr_t)P.self;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    dev_params_c* p = (dev_params_c*)(uintptr_t)(((uint64_t)hi << 32) | lo);
    asm volatile("" : "+s"(p));
    __builtin_assume(p != nullptr);      // CV() then drops its by-value alternative
    return p;
  }
}
#endif
#define SALP_CONSTS [[maybe_unused]] dev_params_c* const PC_ = open_consts<STD>(P)
#define CV(name) (STD ? StdConsts::name : (PC_ ? PC_->name : P.name))

// SoA state rows (device layout; distinct from the public snapshot layout)
enum { SF_X = 0, SF_Y, SF_VX, SF_VY, SF_TH, SF_OM, SF_NOZ, SF_WATER, SF_EPRET, SF_FOOD0 };
enum { SI_PACKED = 0, SI_SSF, SI_FC, SI_RNG, SI_EPLEN, SI_COUNT };

struct DevState {
  double* f;     // [SF_FOOD0 + 2F][pitch]
  int32_t* i;    // [SI_COUNT][pitch]
};

struct DevStats {  // one replica = 16 x 8 B (one 128-B line)
  unsigned long long v[16];
};
enum { ST_STEPS = 0, ST_EPISODES, ST_TERM, ST_TRUNC, ST_COLL, ST_FOOD, ST_EPLEN, ST_REWARD, ST_EPRET };
#define SALP_STATS_REPLICAS 64
#define SALP_FIXED_SCALE 1048576.0  /* 2^20 */

// ------------------------------------------------------------------ host side: salp_config_t -> DevParams
// The reference's defaults (snake:29-33 kwargs, legacy:32-53 constants): what salp_config_default() hands out.
inline void default_config(salp_config_t* c) {
  memset(c, 0, sizeof(*c));
  c->struct_size = (uint32_t)sizeof(*c);
  c->width = 800; c->height = 600; c->num_food_items = 5; c->max_observed_food = 3;
  c->max_steps_without_food = 1500; c->forced_breathing = 1; c->random_food_count = 0; c->respawn_food = 1;
  c->food_reward = 10.0; c->collision_penalty = -50.0; c->time_penalty = -0.1; c->efficiency_bonus = 1.0;
  c->proximity_reward_weight = 0.0;
  c->tank_margin = 50.0; c->base_radius = 30.0; c->max_thrust_force = 100.0; c->drag_coefficient = 0.98;
  c->angular_drag = 0.95; c->max_nozzle_angle = 3.141592653589793 / 3; c->nozzle_response_rate = 0.05;
  c->food_radius = 15.0; c->min_food_distance = 80.0;
  c->inhale_duration = 120; c->exhale_duration = 150; c->rest_duration = 60;
}

// The ranges of a config that salp_vec_create accepts.  SALP_OK, or SALP_ERR_INVALID with the reason in *why.
inline int validate(const salp_config_t* c, const char** why) {
  const auto refuse = [why](const char* msg) { *why = msg; return (int)SALP_ERR_INVALID; };
  if (!c) return refuse("config is NULL");
  if (c->struct_size != sizeof(salp_config_t))
    return refuse("salp_config_t.struct_size mismatch (ABI version skew)");
  if (c->width <= 0 || c->height <= 0) return refuse("width/height must be positive");
  if (c->num_food_items < 0 || c->num_food_items > SALP_MAX_FOOD)
    return refuse("num_food_items must be in [0, SALP_MAX_FOOD]");
  if (c->max_observed_food < 0 || c->max_observed_food > SALP_MAX_OBSERVED_FOOD)
    return refuse("max_observed_food must be in [0, SALP_MAX_OBSERVED_FOOD]");
  if (c->inhale_duration < 1 || c->inhale_duration > 255 || c->exhale_duration < 4 || c->exhale_duration > 254)
    return refuse("inhale_duration in [1,255], exhale_duration in [4,254] required");
  if (c->rest_duration < 0) return refuse("rest_duration must be >= 0");
  if (!(c->base_radius > 0) || !(c->max_nozzle_angle > 0))
    return refuse("base_radius and max_nozzle_angle must be positive");
  return (int)SALP_OK;
}

// The ranges of include/salp_vec.h ("Ranges accepted by salp_vec_set_state"), on a host snapshot of n envs (either array
// may be NULL).  SALP_OK, or SALP_ERR_INVALID with the reason, which names the first env outside, in msg.
inline int check_snapshot(int64_t n, const double* f64, const int32_t* i32, char* msg, size_t msg_size) {
  if (f64) {
    for (int64_t i = 0; i < n; ++i) {
      const double th = f64[SALP_F_THETA * n + i], om = f64[SALP_F_OMEGA * n + i], w = f64[SALP_F_WATER * n + i];
      if (!(fabs(th) <= SALP_SET_STATE_MAX_ANGLE) || !(fabs(om) <= SALP_SET_STATE_MAX_ANGLE)) {
        snprintf(msg, msg_size, "set_state: env %lld: theta %g / omega %g outside [-%g, %g] (or NaN)", (long long)i, th, om,
                 SALP_SET_STATE_MAX_ANGLE, SALP_SET_STATE_MAX_ANGLE);
        return (int)SALP_ERR_INVALID;
      }
      if (!(w >= 0.0 && w <= 1.0)) {
        snprintf(msg, msg_size, "set_state: env %lld: water %.17g outside [0, 1] (or NaN)", (long long)i, w);
        return (int)SALP_ERR_INVALID;
      }
    }
  }
  if (i32) {
    for (int64_t i = 0; i < n; ++i) {
      const int32_t ph = i32[SALP_I_PHASE * n + i], tm = i32[SALP_I_TIMER * n + i], du = i32[SALP_I_EXHALE_DUR * n + i],
                    ho = i32[SALP_I_SHAPE_HOLD * n + i];
      if (ph < 0 || ph > 2 || tm < 0 || tm > 255 || du < 0 || du > 255 || ho < 0 || ho > 7) {
        snprintf(msg, msg_size, "set_state: env %lld: phase %d / timer %d / exhale duration %d / shape hold %d outside 0..2 / 0..255 / 0..255 / 0..7",
                 (long long)i, ph, tm, du, ho);
        return (int)SALP_ERR_INVALID;
      }
    }
  }
  return (int)SALP_OK;
}

inline DevParams make_params(const salp_config_t& c, int64_t n, int64_t pitch, uint64_t seed, int64_t base) {
  DevParams P;
  memset(&P, 0, sizeof(P));
  P.W = (double)c.width; P.H = (double)c.height;
  P.half_W = (double)c.width / 2; P.half_H = (double)c.height / 2;
  P.margin = c.tank_margin;
  P.wall_hi_x = (double)c.width - c.tank_margin; P.wall_hi_y = (double)c.height - c.tank_margin;
  P.R = c.base_radius;
  P.a_rest = c.base_radius * 1.3; P.b_rest = c.base_radius * 0.8; P.ab_full = c.base_radius * 1.1;
  P.da_inh = P.ab_full - P.a_rest; P.db_inh = P.ab_full - P.b_rest;
  P.da_exh = P.a_rest - P.ab_full; P.db_exh = P.b_rest - P.ab_full;
  P.max_nozzle = c.max_nozzle_angle; P.nozzle_rate = c.nozzle_response_rate;
  P.thrust_force = c.max_thrust_force; P.drag = c.drag_coefficient; P.ang_drag = c.angular_drag;
  P.exhale_dur_d = (double)c.exhale_duration;
  P.food_radius = c.food_radius; P.min_food_dist2 = c.min_food_distance * c.min_food_distance;
  P.food_xlo = c.tank_margin + c.food_radius;
  P.food_xspan = ((double)c.width - c.tank_margin - c.food_radius) - P.food_xlo;
  P.food_ylo = P.food_xlo;
  P.food_yspan = ((double)c.height - c.tank_margin - c.food_radius) - P.food_ylo;
  P.food_reward = c.food_reward; P.collision_penalty = c.collision_penalty;
  P.time_penalty = c.time_penalty; P.efficiency_bonus = c.efficiency_bonus;
  P.prox_w = c.proximity_reward_weight;
  P.inv_W = 1.0 / P.W; P.inv_H = 1.0 / P.H; P.inv_pi = 1.0 / 3.141592653589793;
  P.inv_R = 1.0 / c.base_radius; P.inv_max_nozzle = 1.0 / c.max_nozzle_angle;
  P.inv_diag = (float)(1.0 / sqrt(P.W * P.W + P.H * P.H));
  { const double L = P.W > P.H ? P.W : P.H; P.tie_c0 = (float)(1.4e-7 * L * L); }
  P.inhale_dur = c.inhale_duration; P.exhale_dur = c.exhale_duration;
  P.cycle_len = c.inhale_duration + c.exhale_duration + c.rest_duration;
  P.max_steps_wo_food = c.max_steps_without_food;
  P.F = c.num_food_items; P.K = c.max_observed_food;
  P.F_base = c.num_food_items;
  P.forced = c.forced_breathing != 0; P.random_food_count = c.random_food_count != 0;
  P.respawn = c.respawn_food != 0;
  P.autoreset = c.no_autoreset == 0;
  P.seed = nullptr;   // set by salp_vec_create once the ColdBlock exists
  P.env_base = (uint64_t)base; P.n = n; P.pitch = pitch;
  return P;
}

// True when every constant of DevParams equals its StdConsts literal (the reference's defaults).
inline bool is_std(const DevParams& P) {
#define SALP_STD_EQUAL(type, name, literal) && P.name == StdConsts::name
  return true SALP_STD_CONSTS(SALP_STD_EQUAL);
#undef SALP_STD_EQUAL
}

}  // namespace salp
