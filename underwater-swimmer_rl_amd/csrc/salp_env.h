// salp_env.h — one env of the snake simulator in registers: the wavefront's LDS hand-over, EnvCore / Env with their loads
// and stores, the env's draw stream, the ellipse implied by a state, and reset with the serial food placement.
// Device code only; the numerics contract is in salp_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "salp_params.h"       // DevParams, DevState, SF_* / SI_*, CV, pack_breath / bw_*
#include "salp_philox.h"       // U4, philox4x32_10, u53
#include "salp_snake_math.h"   // is_none

namespace salp {

// The wavefront's LDS hand-over: what every lane wrote before is visible to every lane after, and the compiler moves no LDS
// access across it (a wavefront runs in lockstep: the barrier itself is no instruction).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Everything of one env except the food positions.
struct EnvCore {
  double x, y, vx, vy, th, om, noz, water, epret;
  uint32_t packed;
  int ssf, fc, eplen;
  uint32_t rng;
};
// One env with its food positions in registers (all indexing static).  The multi-food rollout kernel
// keeps the foods in LDS instead (salp_food_lds.h) and only an EnvCore in registers.
template <int FMAX>
struct Env : EnvCore {
  double fx[FMAX], fy[FMAX];
};

__device__ __forceinline__ void load_core(EnvCore& e, const DevState& S, const DevParams& P, int64_t i) {
  const int64_t p = P.pitch;
  e.x = S.f[SF_X * p + i]; e.y = S.f[SF_Y * p + i];
  e.vx = S.f[SF_VX * p + i]; e.vy = S.f[SF_VY * p + i];
  e.th = S.f[SF_TH * p + i]; e.om = S.f[SF_OM * p + i];
  e.noz = S.f[SF_NOZ * p + i]; e.water = S.f[SF_WATER * p + i];
  e.epret = S.f[SF_EPRET * p + i];
  e.packed = (uint32_t)S.i[SI_PACKED * p + i];
  e.ssf = S.i[SI_SSF * p + i]; e.fc = S.i[SI_FC * p + i];
  e.rng = (uint32_t)S.i[SI_RNG * p + i]; e.eplen = S.i[SI_EPLEN * p + i];
}
__device__ __forceinline__ void store_core(const EnvCore& e, const DevState& S, const DevParams& P, int64_t i) {
  const int64_t p = P.pitch;
  S.f[SF_X * p + i] = e.x; S.f[SF_Y * p + i] = e.y;
  S.f[SF_VX * p + i] = e.vx; S.f[SF_VY * p + i] = e.vy;
  S.f[SF_TH * p + i] = e.th; S.f[SF_OM * p + i] = e.om;
  S.f[SF_NOZ * p + i] = e.noz; S.f[SF_WATER * p + i] = e.water;
  S.f[SF_EPRET * p + i] = e.epret;
  S.i[SI_PACKED * p + i] = (int32_t)e.packed;
  S.i[SI_SSF * p + i] = e.ssf; S.i[SI_FC * p + i] = e.fc;
  S.i[SI_RNG * p + i] = (int32_t)e.rng; S.i[SI_EPLEN * p + i] = e.eplen;
}

template <int FMAX>
__device__ __forceinline__ void load_env(Env<FMAX>& e, const DevState& S, const DevParams& P, int64_t i) {
  const int64_t p = P.pitch;
  load_core(e, S, P, i);
#pragma unroll
  for (int k = 0; k < FMAX; ++k) {
    if (k < P.F) {
      e.fx[k] = S.f[(SF_FOOD0 + k) * p + i];
      e.fy[k] = S.f[(SF_FOOD0 + P.F + k) * p + i];
    } else {
      e.fx[k] = __builtin_nan(""); e.fy[k] = __builtin_nan("");
    }
  }
}

template <int FMAX>
__device__ __forceinline__ void store_env(const Env<FMAX>& e, const DevState& S, const DevParams& P, int64_t i) {
  const int64_t p = P.pitch;
  store_core(e, S, P, i);
#pragma unroll
  for (int k = 0; k < FMAX; ++k) {
    if (k < P.F) {
      S.f[(SF_FOOD0 + k) * p + i] = e.fx[k];
      S.f[(SF_FOOD0 + P.F + k) * p + i] = e.fy[k];
    }
  }
}

// One Philox block of this env's draw stream (include/salp_vec.h "Randomness").
__device__ __forceinline__ U4 next_block(EnvCore& e, const DevParams& P, uint64_t genv) {
  // The key is made opaque here: otherwise the 18 round keys (seed + r * Weyl constant) are hoisted out of the
  // step loop as loop invariants, spilled to VGPR lanes and read back with v_readlane on every use — two
  // scalar adds per round in place are cheaper.
  uint32_t k0 = P.seed[0], k1 = P.seed[1];
  asm volatile("" : "+s"(k0), "+s"(k1));
  U4 w = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), e.rng, 0u, k0, k1);
  e.rng += 1u;
  return w;
}

template <int FMAX, bool STD>
__device__ __forceinline__ void draw_xy(EnvCore& e, const DevParams& P, uint64_t genv, double& x, double& y) {
  SALP_CONSTS;
  const U4 w = next_block(e, P, genv);
  x = CV(food_xlo) + CV(food_xspan) * u53(w.x, w.y);
  y = CV(food_ylo) + CV(food_yspan) * u53(w.z, w.w);
}

// Ellipse semi-axes implied by the post-step state (see SALP_I_SHAPE_HOLD in salp_vec.h).
template <bool STD>
__device__ __forceinline__ void shape_of(const DevParams& P, uint32_t packed, double water, double& a, double& b) {
  SALP_CONSTS;
  const int phase = bw_phase(packed), timer = bw_timer(packed), dur = bw_dur(packed), hold = bw_hold(packed);
  if (hold == 7) { a = CV(R); b = CV(R); return; }
  if (hold != 0) {
    const double p = (double)hold / (double)CV(inhale_dur);
    a = CV(a_rest) + CV(da_inh) * p; b = CV(b_rest) + CV(db_inh) * p; return;
  }
  if (phase == 0) { a = CV(a_rest); b = CV(b_rest); }
  else if (phase == 1 || timer == 0) { a = CV(a_rest) + CV(da_inh) * water; b = CV(b_rest) + CV(db_inh) * water; }
  else {
    const double p = (double)timer / (double)dur;
    a = CV(ab_full) + CV(da_exh) * p; b = CV(ab_full) + CV(db_exh) * p;
  }
}

// Food placement, shared by reset (snake:92-131 _generate_food_positions) and respawn
// (snake:232-276 _respawn_food).  Both are the same rejection sampler: draw (x, y); reject if within
// min_food_distance of a live food or of the robot — at reset the robot sits at the tank centre,
// which is the point snake:115 tests against — and after `limit` rejections (100 at reset, 50 at
// respawn) accept the next draw unconditionally.  The accepted point fills the first empty slot
// (at reset slots fill in order, snake:120; at respawn snake:261-264).  `todo` = foods still to place.
template <int FMAX, bool STD>
__device__ __forceinline__ void place_food(Env<FMAX>& e, const DevParams& P, uint64_t genv, int todo, int limit) {
  SALP_CONSTS;
  int attempts = 0;
#pragma unroll 1
  while (__any(todo > 0)) {
    if (todo > 0) {
      double x, y;
      draw_xy<FMAX, STD>(e, P, genv, x, y);
      bool valid = true;
      {
        const double dx = x - e.x, dy = y - e.y;
        if (dx * dx + dy * dy < CV(min_food_dist2)) valid = false;
      }
#pragma unroll
      for (int k = 0; k < FMAX; ++k) {
        const double dx = x - e.fx[k], dy = y - e.fy[k];
        if (dx * dx + dy * dy < CV(min_food_dist2)) valid = false;   // NaN (empty) slots never reject
      }
      if (valid || attempts >= limit) {
        bool put = false;
#pragma unroll
        for (int k = 0; k < FMAX; ++k) {
          if (!put && k < P.F && is_none(e.fx[k])) { e.fx[k] = x; e.fy[k] = y; put = true; }
        }
        todo -= 1;
        attempts = 0;
      } else {
        attempts += 1;
      }
    }
  }
}

// legacy:95-117 reset + snake:133-149 (pose, breathing, counters, episode food count); the food
// itself is placed by place_food(e, ..., todo = return value, limit = 100).
// F_base: base_num_food_items of this launch (the one constant a caller may change between launches).
template <bool STD>
__device__ __forceinline__ int reset_core(EnvCore& e, const DevParams& P, uint64_t genv, int F_base) {
  SALP_CONSTS;
  e.x = CV(half_W); e.y = CV(half_H); e.vx = 0.0; e.vy = 0.0; e.th = 0.0; e.om = 0.0;
  e.noz = 0.0; e.water = 0.0; e.epret = 0.0;
  e.packed = pack_breath(0, 0, bw_dur(e.packed), 7);
  e.ssf = 0; e.fc = 0; e.eplen = 0;
  int nf = F_base;
  if (P.random_food_count) {  // snake:146 random.randint(1, max(1, base))
    const U4 w = next_block(e, P, genv);
    const uint32_t n = (uint32_t)(F_base > 1 ? F_base : 1);
    nf = 1 + (int)(((uint64_t)w.x * (uint64_t)n) >> 32);
    if (nf > P.F) nf = P.F;
  }
  return nf;
}
template <int FMAX, bool STD>
__device__ __forceinline__ int reset_pose(Env<FMAX>& e, const DevParams& P, uint64_t genv, int F_base) {
  const int nf = reset_core<STD>(e, P, genv, F_base);
#pragma unroll
  for (int k = 0; k < FMAX; ++k) { e.fx[k] = __builtin_nan(""); e.fy[k] = __builtin_nan(""); }
  return nf;
}

}  // namespace salp
