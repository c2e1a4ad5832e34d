// salp_step.h — one reference step of a snake env with its food in registers, and its observation row: the jet thrust,
// the nearest food, step_head / step_tail / step_env, observe.  The multi-food rollout kernels share step_head and
// step_tail and select their foods through salp_food_reg.h / salp_food_lds.h.  Device code only; the numerics contract is
// in salp_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "salp_exp.h"          // SALP_STAMP*
#include "salp_env.h"          // EnvCore, Env, next_block; through it salp_params.h, salp_philox.h
#include "salp_snake_math.h"   // thrust table, sincos_small_t, sin_nozzle_t, relative_heading, cos_wrapped

namespace salp {

// legacy:261-314 _apply_jet_thrust (water is the value BEFORE this step's decay).
// The reference evaluates cos/sin at three angles: phi, fl(phi + pi/2) and fl(phi + jitter).  One
// sincos(phi) serves all three: the side angle is a quarter turn plus the (exactly recovered)
// rounding error of the addition, the jitter angle a rotation by |D| <= 0.025 (short series).
// The seven increments of one thrust step, in the order legacy:261-314 applies them:
//   vx = ((vx + t.ax) + t.bx) + t.cx,  vy likewise,  omega = omega + t.om
// (main jet, side thrust, jitter).  A function of (theta, nozzle, water before this step's decay, r = max(a, b),
// the env's draw counter and global index) only.
struct ThrustTerms { double ax, ay, bx, by, cx, cy, om; };
template <bool STD>
__device__ __forceinline__ ThrustTerms jet_thrust_terms(double th, double noz, double water, double r, uint32_t rng,
                                                        uint64_t genv, const DevParams& P) {
  SALP_CONSTS;
  ThrustTerms t;
  tbl_double* TT = thrust_table();
  const double T = mul_s(CV(thrust_force) * water, TT[TT_K04]);
  const double phi = th - noz;
  double s, c;
  sincos_small_t(TT, phi, s, c);
  t.ax = mul_s(c * T, TT[TT_K012]);
  t.ay = mul_s(s * T, TT[TT_K012]);
  const double nn = -noz;
  const double primary = mul_s(nn * T, TT[TT_K0002]);
  const double arm = r * TT[TT_K07];
  const double perp = T * sin_nozzle_t(TT, nn);
  const double moment = mul_s(perp * arm, TT[TT_K00005]);
  const double shape = mul_s((nn * T) * water, TT[TT_K00003]);
  t.om = (primary + moment) + shape;
  {  // side thrust at fl(phi + fl(pi/2)) = phi + pi/2 + dl,  dl = fl(pi/2) - pi/2 (6.1e-17) up to the rounding of the sum,
     // ulp(|phi + pi/2|) / 2: 2.2e-16 rad below 2, 4.4e-16 below 4 (a wrapped heading: 4e-17 px per step through the 0.1-px
     // side term, below the device sincos' own last-bit departure from glibc — round 2 recovered it with a TwoSum, six fp64
     // instructions per thrust step), and 7.1e-15 rad up to the |theta| <= 100 that salp_vec_set_state admits before the
     // first step wraps it (7e-16 px).  Measured per term against the reference's formulas: tests/test_gpu_snake_math.py.
    const double dl = TT[TT_DL];
    const double sc = -fma(dl, c, s);     // cos(side) = -sin(phi + dl)
    const double ss = fma(-dl, s, c);     // sin(side) =  cos(phi + dl)
    const double S = mul_s(T * fabs(noz), TT[TT_K03]);
    t.bx = mul_s(sc * S, TT[TT_K008]);
    t.by = mul_s(ss * S, TT[TT_K008]);
  }
  {  // jitter at fl(phi + d), d = fl((u - 0.5) * 0.05); one Philox block of the env's draw stream (counter rng)
    uint32_t k0 = P.seed[0], k1 = P.seed[1], g0 = (uint32_t)genv;
    asm volatile("" : "+s"(k0), "+s"(k1));    // see next_block
    asm volatile("" : "+v"(g0));              // likewise the first-round product 0xD2511F53 * env_lo: one v_mad_u64_u32 here
                                              // instead of a 64-bit VGPR pair held across the step loop
    const U4 w = philox4x32_10(g0, (uint32_t)(genv >> 32), rng, 0u, k0, k1);
    const double u = u53(w.x, w.y);
    const double d = mul_s(u - 0.5, TT[TT_K005]);
    const double D = d;                   // fl(phi + d) = phi + D up to the sum's rounding, ulp(|phi + d|) / 2 as above (<= 4.4e-16
                                          // rad for a wrapped heading, 7.1e-15 at |theta| = 100, on a 3e-3-px term); the series drop
                                          // D^11 / 11! and D^10 / 10! (< 3e-23 at |D| <= 0.025)
    const double z = D * D;
    double sp = fma_s(z, (double)TT[TT_J_S3], TT[TT_J_S2]);
    sp = fma_s(z, sp, TT[TT_J_S1]);
    sp = fma_s(z, sp, TT[TT_J_S0]);
    const double sD = fma(D * z, sp, D);
    double cp = fma_s(z, (double)TT[TT_J_C3], TT[TT_J_C2]);
    cp = fma_s(z, cp, TT[TT_J_C1]);
    cp = fma(z, cp, -0.5);
    const double cD = fma(z, cp, 1.0);
    const double nc = c * cD - s * sD;
    const double ns = s * cD + c * sD;
    const double nf = T * TT[TT_K004];
    t.cx = mul_s(nc * nf, TT[TT_K0002J]);
    t.cy = mul_s(ns * nf, TT[TT_K0002J]);
  }
  return t;
}
__device__ __forceinline__ void apply_thrust_terms(EnvCore& e, const ThrustTerms& t) {
  e.vx = ((e.vx + t.ax) + t.bx) + t.cx;
  e.vy = ((e.vy + t.ay) + t.by) + t.cy;
  e.om = e.om + t.om;
  e.rng += 1u;
}
// legacy:261-314 _apply_jet_thrust (water is the value BEFORE this step's decay), the lane serving itself.
template <int FMAX, bool STD>
__device__ __forceinline__ void apply_jet_thrust(EnvCore& e, const DevParams& P, uint64_t genv, double r) {
  apply_thrust_terms(e, jet_thrust_terms<STD>(e.th, e.noz, e.water, r, e.rng, genv, P));
}

// (Two experiments that lived here are gone from the source, their measurements are in profiles/r02/ab_notes.md and
// their code in the history: a block-pooled thrust — one wavefront evaluating the thrust of a workgroup's four
// between two barriers, bit-identical and 35 % slower, session 6 — and the step's fp64 constants pinned in VGPRs —
// -1.8 % at equal residency, +5 % once its 217 VGPRs cost the third wavefront per SIMD, session 3.)

// Geometry of the nearest live food (first minimum, snake:350-364) in fp64 state terms.
struct Nearest {
  double dx, dy, d2;
  bool any;
};
template <int FMAX>
__device__ __forceinline__ Nearest nearest_food(const Env<FMAX>& e) {
  Nearest g;
  g.dx = 0.0; g.dy = 0.0; g.d2 = 0.0; g.any = false;
#pragma unroll
  for (int k = 0; k < FMAX; ++k) {
    const double dx = e.fx[k] - e.x, dy = e.fy[k] - e.y;
    const double d2 = dx * dx + dy * dy;
    if (!is_none(e.fx[k]) && (!g.any || d2 < g.d2)) { g.any = true; g.d2 = d2; g.dx = dx; g.dy = dy; }
  }
  return g;
}

struct StepOut {
  double rmax;    // max(ellipse_a, ellipse_b) of this step
  float reward;
  float rel;      // relative heading of the nearest food used by the reward (valid if rel_valid)
  bool rel_valid; // the reward evaluated `rel` for the food set that observe() will also see
  bool terminated, truncated, collision, collected;
};

// One reference step (legacy:119-156 under snake:157-189), without autoreset / observation.
// The respawn of a collected food (snake:179-180) is left to the caller — place_food(todo = 1,
// limit = 50) when o.collected && P.respawn, BEFORE any autoreset so the draw order of the
// reference is kept.  (The all-collected termination test only applies when !P.respawn.)
// legacy:119-156 up to and including the wall bounce; returns r = max(ellipse_a, ellipse_b) of this step.
template <bool FORCED, bool STD>
__device__ __forceinline__ double step_head(EnvCore& e, const DevParams& P, uint64_t genv, float a0, float a1 SALP_STAMP_PARAM) {
  SALP_CONSTS;
  int phase = bw_phase(e.packed), timer = bw_timer(e.packed), dur = bw_dur(e.packed);
  // legacy:121-135
  double nd;
  bool inhaling;
  if (FORCED) {
    nd = (double)a0;
    const int tm = (CV(cycle_len) > 255) ? timer : (timer % CV(cycle_len));
    inhaling = tm < CV(inhale_dur);
  } else {
    inhaling = a0 > 0.5f;
    nd = (double)a1;
  }
  const double max_noz = CV(max_nozzle), noz_rate = CV(nozzle_rate);
  const double target = nd * max_noz;
  // legacy:169-182 _update_nozzle
  {
    const double diff = target - e.noz;
    double nz;
    if (fabs(diff) > noz_rate) nz = (diff > 0) ? (e.noz + noz_rate) : (e.noz - noz_rate);
    else nz = target;
    e.noz = pymax(-max_noz, pymin(max_noz, nz));
  }
  // legacy:184-259 _update_breathing_cycle
  double a, b;
  int hold = 0;
  bool thrust = false;
  double water_next = e.water;
  {
    const int tnew = timer + 1;
    const double den = (phase == 2) ? (double)dur : (double)CV(inhale_dur);
    // p = tnew / den, correctly rounded, without the fp64 division sequence (~14 VALU incl. v_rcp_f64): with
    // y = RN(1 / den), q0 = RN(tnew y), r = tnew - den q0 (exact in an fma), RN(q0 + r y) is the IEEE quotient
    // (Markstein) — checked exhaustively for every den in 1..255 and tnew in 1..257.  y is a constant for the
    // inhale duration and for a full exhale (dur = exhale_duration, every exhale of forced breathing); lanes
    // whose exhale was cut short (dur from the water level, legacy:223) divide once to get theirs.
    double yden = (phase == 2) ? (1.0 / (double)CV(exhale_dur)) : (1.0 / (double)CV(inhale_dur));
    {
      const bool odd = (phase == 2) && (dur != CV(exhale_dur));
      if (__any(odd)) {
        asm volatile("" ::: "memory");   // keeps the division inside the (wave-uniform) branch: not speculated
        if (odd) yden = 1.0 / (double)dur;
      }
    }
    const double a_rest = CV(a_rest), b_rest = CV(b_rest), da_inh = CV(da_inh), db_inh = CV(db_inh);
    const double ab_full = CV(ab_full), da_exh = CV(da_exh), db_exh = CV(db_exh);
    const double tn = (double)tnew;
    const double q0 = tn * yden;
    const double p = fma(fma(-den, q0, tn), yden, q0);   // == (double)tnew / den, tests/test_source_claims.py
    if (phase == 0) {
      a = a_rest; b = b_rest;
      if (inhaling) { phase = 1; timer = 0; }
    } else if (phase == 1) {
      if (inhaling && timer < CV(inhale_dur)) {
        timer = tnew;
        a = a_rest + da_inh * p; b = b_rest + db_inh * p;
        water_next = p;
      } else {
        a = a_rest + da_inh * e.water; b = b_rest + db_inh * e.water;  // unchanged ellipse
        if (e.water > 0.05) {
          phase = 2; timer = 0;
          dur = (int)(CV(exhale_dur_d) * pymax(e.water, 0.3));
        } else {
          hold = (timer >= 1 && timer <= 6) ? timer : 0;
          phase = 0; timer = 0; water_next = 0.0;
        }
      }
    } else {
      if (p <= 1.0) {
        timer = tnew;
        a = ab_full + da_exh * p; b = ab_full + db_exh * p;
        thrust = (0.1 <= p) && (p <= 0.5);
        const double v = e.water * (1.0 - p);
        water_next = (v > 0) ? v : 0.0;
      } else {
        a = ab_full + da_exh * 1.0; b = ab_full + db_exh * 1.0;  // ellipse of the last exhale step
        phase = 0; timer = 0; water_next = 0.0;
      }
    }
  }
  // max(ellipse_a, ellipse_b) is ellipse_a whenever both come from the formulas above with the reference's radii:
  // a - b = R (0.5 - 0.5 p) inhaling, R 0.5 p exhaling, 0.5 R at rest, all >= 0 and exact in fp64 for R = 30 (a and b
  // are multiples of 2^-46 below 64: every product and sum above is exact or rounds both the same way is NOT assumed —
  // checked for every (phase, timer, duration) of the literal constants by tests/test_source_claims.py).  In the release
  // branch a and b come from the state's water level w itself, whatever put it there: fl(-6 w) >= -6 and fl(9 w) <= 9 for
  // w in [0, 1] and rounding is monotonic, so a >= 33 >= b — salp_vec_set_state refuses a water level outside [0, 1].
  // Other radii keep the maximum.
  const double r = STD ? a : pymax(a, b);
#ifdef SALP_EXP_NO_THRUST      // experiment build (profiles/ab_bench.py): price of the thrust block
  thrust = false;
#endif
  SALP_STAMP(1);
  if (thrust) apply_jet_thrust<1, STD>(e, P, genv, r);
  SALP_STAMP(2);
  e.water = water_next;
  e.packed = pack_breath(phase, timer, dur, hold);
  // legacy:316-352 _update_physics
  e.vx = e.vx * CV(drag); e.vy = e.vy * CV(drag); e.om = e.om * CV(ang_drag);
  e.x = e.x + e.vx; e.y = e.y + e.vy; e.th = e.th + e.om;
  // legacy:329-332 `while theta > pi: theta -= 2 pi` / `while theta < -pi: ...`.  |omega| is far below
  // 2 pi, so one conditional step each is the common case; the loops only run if a lane is still outside,
  // after an injected state.  They subtract as the reference does (same roundings) and are bounded so that no state
  // can hang a wavefront: salp_vec_set_state admits |theta|, |omega| <= 100 (include/salp_vec.h), so |theta + omega|
  // <= 200 + pi needs at most 33 turns.
  const double pi = SALP_PI, twopi = SALP_2PI;
  if (e.th > pi) e.th -= twopi;
  if (e.th < -pi) e.th += twopi;
  if (__any(e.th > pi || e.th < -pi)) {
#pragma unroll 1
    for (int it = 0; it < 64 && e.th > pi; ++it) e.th -= twopi;
#pragma unroll 1
    for (int it = 0; it < 64 && e.th < -pi; ++it) e.th += twopi;
  }
  {
    const double m = CV(margin) + r;
    const double hx = CV(W) - m, hy = CV(H) - m;
    const double k04 = 0.4, k07 = 0.7;
    if (e.x < m) { e.x = m; e.vx = fabs(e.vx) * k04; e.om = e.om * k07; }
    else if (e.x > hx) { e.x = hx; e.vx = -fabs(e.vx) * k04; e.om = e.om * k07; }
    if (e.y < m) { e.y = m; e.vy = fabs(e.vy) * k04; e.om = e.om * k07; }
    else if (e.y > hy) { e.y = hy; e.vy = -fabs(e.vy) * k04; e.om = e.om * k07; }
  }
  SALP_STAMP(3);
  return r;
}

// snake:171-189 counters and termination, given the step's reward so far (everything but the counters)
// and whether any food is still alive (only read when !P.respawn).
__device__ __forceinline__ void step_tail(EnvCore& e, const DevParams& P, StepOut& o, double rew, bool any_alive) {
  e.ssf += 1;
  if (o.collected) {
    e.fc += 1;
    e.ssf = 0;
    o.rel_valid = false;  // the food set changed after the reward was computed
  }
  o.terminated = false; o.truncated = false;
  if (o.collision) o.terminated = true;
  else if (e.ssf > P.max_steps_wo_food) o.truncated = true;
  else if (!P.respawn && !any_alive) o.terminated = true;
  e.eplen += 1;
  e.epret += rew;
  o.reward = (float)rew;
}

template <int FMAX, bool FORCED, bool STD>
__device__ __forceinline__ StepOut step_env(Env<FMAX>& e, const DevParams& P, uint64_t genv, float a0, float a1 SALP_STAMP_PARAM) {
  SALP_CONSTS;
  const double r = step_head<FORCED, STD>(e, P, genv, a0, a1 SALP_STAMP_PASS);
  StepOut o;
  o.rmax = r;
  // snake:204-217 _check_food_collection (first live food inside the capture radius)
  o.collected = false;
  {
    const double cr = r + CV(food_radius);
    const double cr2 = cr * cr;
#pragma unroll
    for (int k = 0; k < FMAX; ++k) {
      const double dx = e.x - e.fx[k], dy = e.y - e.fy[k];
      if constexpr (FMAX == 1) {
        if (!o.collected && (dx * dx + dy * dy < cr2)) {
          o.collected = true; e.fx[k] = __builtin_nan(""); e.fy[k] = __builtin_nan("");
        }
      } else {   // multi-food: selects instead of branches
        const bool hit = !o.collected && (dx * dx + dy * dy < cr2);
        e.fx[k] = hit ? __builtin_nan("") : e.fx[k];
        e.fy[k] = hit ? __builtin_nan("") : e.fy[k];
        o.collected = o.collected || hit;
      }
    }
  }
  // snake:219-230 _check_wall_collision
  o.collision = (e.x - r <= CV(margin)) || (e.x + r >= CV(wall_hi_x)) || (e.y - r <= CV(margin)) || (e.y + r >= CV(wall_hi_y));
  // snake:278-327 _calculate_snake_reward
  double rew = 0.0;
  if (o.collected) {
    rew += P.food_reward;
    if (P.efficiency_bonus > 0) rew += P.efficiency_bonus * (double)(P.max_steps_wo_food - e.ssf);
  }
  if (o.collision) rew += P.collision_penalty;
  o.rel = 0.f; o.rel_valid = false;
  if (P.prox_w > 0) {
    const Nearest g = nearest_food(e);
    if (g.any) {
      // alignment = cos(wrap(atan2(dy,dx) - theta)); fp32 is enough for a term that only leaves
      // the simulator (snake:301-322).  The heading is handed to observe() for reuse.
      o.rel = relative_heading<true>((float)g.dy, (float)g.dx, (float)e.th);
      o.rel_valid = true;
      rew += P.prox_w * (double)cos_wrapped(o.rel);
    }
  }
  rew += P.time_penalty;
  bool any_alive = false;
  if (!P.respawn) {
#pragma unroll
    for (int k = 0; k < FMAX; ++k) any_alive = any_alive || !is_none(e.fx[k]);
  }
  step_tail(e, P, o, rew, any_alive);
  SALP_STAMP(5);
  return o;
}

// legacy:371-388 + snake:366-428: the observation row (10 + 4K + 2 floats) in registers `o`.
// rmax = max(ellipse_a, ellipse_b) of the current state.  If have_rel, `rel0` is the relative
// heading of the nearest food already evaluated by the reward for the same food set.
template <int FMAX, int KMAX, bool STD>
__device__ __forceinline__ void observe(const Env<FMAX>& e, const DevParams& P, double rmax, bool have_rel, float rel0,
                                        float (&o)[12 + 4 * KMAX]) {
  SALP_CONSTS;
  const int K = (KMAX == 3) ? 3 : P.K;
  // normalisations in fp32 on the rounded fp64 state (<= 1.5 ulp of the reference's f32 value)
  o[0] = (float)e.x * (float)CV(inv_W);
  o[1] = (float)e.y * (float)CV(inv_H);
  o[2] = (float)e.vx * 0.2f;
  o[3] = (float)e.vy * 0.2f;
  o[4] = (float)e.th * (float)CV(inv_pi);
  o[5] = (float)e.om * 10.0f;
  o[6] = (float)rmax * (float)CV(inv_R);
  o[7] = (float)bw_phase(e.packed) * 0.5f;
  o[8] = (float)e.water;
  o[9] = (float)e.noz * (float)CV(inv_max_nozzle);
  float dsum = 0.f;
  int cnt = 0;
  if constexpr (FMAX == 1) {
  // squared distances of live foods in fp64 (the sort key), distances in fp32 (the outputs)
  double d2[FMAX];
  float d[FMAX];
  uint32_t live = 0;
#pragma unroll
  for (int k = 0; k < FMAX; ++k) {
    const double dx = e.fx[k] - e.x, dy = e.fy[k] - e.y;
    d2[k] = dx * dx + dy * dy;
    const bool ok = !is_none(e.fx[k]);
    d[k] = __builtin_amdgcn_sqrtf((float)d2[k]);
    if (ok) { live |= (1u << k); ++cnt; }
  }
  const float th = (float)e.th;
  // K nearest, nearest first; ties keep slot order (stable sort, snake:382)
  uint32_t left = live;
#pragma unroll
  for (int s = 0; s < KMAX; ++s) {
    float v0 = 0.f, v1 = 0.f, v2 = 1.f, v3 = 0.f;   // padding for an empty slot (snake:412)
    if (s < K) {
      double bd2 = 0.0;
      float bd = 0.f, bx = 0.f, by = 0.f;
      int bi = -1;
#pragma unroll
      for (int k = 0; k < FMAX; ++k) {
        const bool cand = ((left >> k) & 1u) && (bi < 0 || d2[k] < bd2);
        if (cand) { bi = k; bd2 = d2[k]; bd = d[k]; bx = (float)(e.fx[k] - e.x); by = (float)(e.fy[k] - e.y); }
      }
      if (bi >= 0) {
        left &= ~(1u << bi);
        dsum += bd;
        float rel;
        if (s == 0) {
          if (__all(have_rel)) rel = rel0;                    // wave-uniform: skips the second atan2
          else rel = have_rel ? rel0 : relative_heading(by, bx, th);
        } else {
          rel = relative_heading(by, bx, th);
        }
        v0 = bx * (float)CV(inv_W);
        v1 = by * (float)CV(inv_H);
        v2 = bd * CV(inv_diag);
        v3 = rel * 0.318309886183791f;
      }
    }
    o[10 + 4 * s + 0] = v0; o[10 + 4 * s + 1] = v1; o[10 + 4 * s + 2] = v2; o[10 + 4 * s + 3] = v3;
  }
  // the mean distance runs over ALL live foods (snake:418-420), not only the K observed
#pragma unroll
  for (int k = 0; k < FMAX; ++k) if ((left >> k) & 1u) dsum += d[k];
  } else {
  // (reset / observe kernels only: the rollout kernels select through salp_food_reg.h / salp_food_lds.h.)  The sort key
  // is the reference's: the fp64 distance sqrt(dx^2 + dy^2) (snake:378-382; squared distances an ulp apart can share a
  // distance, and then slot order decides); offsets and distances of the outputs in fp32.  Written with selects.
  double d2[FMAX];
  float d[FMAX], dxf[FMAX], dyf[FMAX];
  uint32_t live = 0;
#pragma unroll
  for (int k = 0; k < FMAX; ++k) {
    const double dx = e.fx[k] - e.x, dy = e.fy[k] - e.y;
    const double sq = dx * dx + dy * dy;
    d2[k] = __builtin_sqrt(sq);
    const bool ok = !is_none(e.fx[k]);
    dxf[k] = (float)dx; dyf[k] = (float)dy;
    d[k] = __builtin_amdgcn_sqrtf((float)sq);
    live |= ok ? (1u << k) : 0u;
    cnt += ok ? 1 : 0;
  }
  const float th = (float)e.th;
  // K nearest, nearest first; ties keep slot order (stable sort, snake:382)
  uint32_t left = live;
#pragma unroll
  for (int s = 0; s < KMAX; ++s) {
    float v0 = 0.f, v1 = 0.f, v2 = 1.f, v3 = 0.f;   // padding for an empty slot (snake:412)
    if (s < K) {
      double bd2 = 0.0;
      float bd = 0.f, bx = 0.f, by = 0.f;
      int bi = -1;
#pragma unroll
      for (int k = 0; k < FMAX; ++k) {
        const bool cand = ((left >> k) & 1u) && (bi < 0 || d2[k] < bd2);
        bi = cand ? k : bi;
        bd2 = cand ? d2[k] : bd2;
        bd = cand ? d[k] : bd;
        bx = cand ? dxf[k] : bx;
        by = cand ? dyf[k] : by;
      }
      const bool found = bi >= 0;
      left &= found ? ~(1u << (bi & 31)) : 0xFFFFFFFFu;
      dsum += found ? bd : 0.f;
      float rel;
      if (s == 0 && __all(have_rel)) rel = rel0;              // wave-uniform: skips the second atan2
      else {
        rel = relative_heading(by, bx, th);
        if (s == 0) rel = have_rel ? rel0 : rel;
      }
      v0 = found ? bx * (float)CV(inv_W) : 0.f;
      v1 = found ? by * (float)CV(inv_H) : 0.f;
      v2 = found ? bd * CV(inv_diag) : 1.f;
      v3 = found ? rel * 0.318309886183791f : 0.f;
    }
    o[10 + 4 * s + 0] = v0; o[10 + 4 * s + 1] = v1; o[10 + 4 * s + 2] = v2; o[10 + 4 * s + 3] = v3;
  }
  // the mean distance runs over ALL live foods (snake:418-420), not only the K observed
#pragma unroll
  for (int k = 0; k < FMAX; ++k) dsum += ((left >> k) & 1u) ? d[k] : 0.f;
  }
  const float fcnt = (float)cnt;
  const float s0 = fminf(fcnt * 0.1f, 1.0f);
  const float s1 = (cnt > 0) ? (dsum * __builtin_amdgcn_rcpf(fcnt)) * CV(inv_diag) : 1.0f;
  // the two summary values sit right after the K-th food block
  if (KMAX == 3) {
    o[22] = s0; o[23] = s1;
  } else {
#pragma unroll
    for (int s = 0; s <= KMAX; ++s) if (s == K) { o[10 + 4 * s] = s0; o[11 + 4 * s] = s1; }
  }
}

}  // namespace salp
