// salp_service_kernels.h — the service kernels of the snake library, everything on the device that is not the fused
// step/rollout kernel (salp_rollout_kernel.h): generated actions, reset / observe, the state snapshots, reseed, and the
// policy relayout and noise step; and the math probe of the tests.  Included by salp_vec.hip alone, which launches them;
// device code only.
#pragma once
#include "salp_rollout_kernel.h"   // through it: DevParams / DevState / ColdBlock, Env, the draw streams, PH_*, kBlock
#include "salp_snake_math_probe.h" // SALP_SNAKE_MATH_*

namespace {

// Device-generated actions (salp_vec_rollout with act == NULL): a[t][env][j] from the env's
// action stream, Philox counter (env_lo, env_hi, global_step + t, 1 + j).
__global__ __launch_bounds__(kBlock) void salp_gen_actions_kernel(DevParams P, float* act, int H, int AD, int64_t global_step) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= P.n) return;
  const uint64_t genv = P.env_base + (uint64_t)i;
  U4 w = {0u, 0u, 0u, 0u}, w2 = {0u, 0u, 0u, 0u};
  for (int t = 0; t < H; ++t) {
    const uint32_t ts = (uint32_t)(global_step + t);
    if (t == 0 || (ts & 3u) == 0u) {
      w = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), ts >> 2, 1u, P.seed[0], P.seed[1]);
      if (AD == 2) w2 = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), ts >> 2, 2u, P.seed[0], P.seed[1]);
    }
    const uint32_t k = ts & 3u;
    const uint32_t x0 = (k == 0) ? w.x : (k == 1) ? w.y : (k == 2) ? w.z : w.w;
    const uint32_t x1 = (k == 0) ? w2.x : (k == 1) ? w2.y : (k == 2) ? w2.z : w2.w;
    const int64_t o = ((int64_t)t * P.n + i) * AD;
    if (AD == 1) {
      act[o] = (float)(x0 >> 8) * 1.1920928955078125e-7f - 1.0f;
    } else {
      act[o] = (float)(x0 >> 8) * 5.9604644775390625e-8f;
      act[o + 1] = (float)(x1 >> 8) * 1.1920928955078125e-7f - 1.0f;
    }
  }
}

// reset(mask) + observation
template <int FMAX, int KMAX, bool STD>
__global__ __launch_bounds__(kBlock) void salp_reset_kernel(DevParams P, DevState S, const uint8_t* mask, float* obs, int do_reset) {
  const int64_t env = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (env >= P.n) return;
  const uint64_t genv = P.env_base + (uint64_t)env;
  Env<FMAX> e;
  load_env(e, S, P, env);
  const bool resetting = do_reset && (!mask || mask[env]);
  int todo = 0;
  if (resetting) {
    const int nf = reset_pose<FMAX, STD>(e, P, genv, P.F_base);
    // place_food loops until no lane of the wavefront has food left to place; lanes that are not
    // being reset pass todo = 0
    todo = nf;
  }
  place_food<FMAX, STD>(e, P, genv, todo, 100);
  if (resetting) {
    store_env(e, S, P, env);
  }
  if (obs) {
    const int K = (KMAX == 3) ? 3 : P.K;
    double a, b;
    shape_of<STD>(P, e.packed, e.water, a, b);
    float ob[12 + 4 * KMAX];
    observe<FMAX, KMAX, STD>(e, P, pymax(a, b), false, 0.f, ob);
    float4* dst = reinterpret_cast<float4*>(obs + env * (12 + 4 * K));
#pragma unroll
    for (int q = 0; q < 3 + KMAX; ++q)
      if (q < 3 + K) dst[q] = make_float4(ob[4 * q], ob[4 * q + 1], ob[4 * q + 2], ob[4 * q + 3]);
  }
}

// public snapshot <-> device layout
__global__ void salp_get_state_kernel(DevParams P, DevState S, double* f64, int32_t* i32) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.n) return;
  const int64_t p = P.pitch, n = P.n;
  const uint32_t packed = (uint32_t)S.i[SI_PACKED * p + i];
  if (f64) {
    f64[SALP_F_X * n + i] = S.f[SF_X * p + i]; f64[SALP_F_Y * n + i] = S.f[SF_Y * p + i];
    f64[SALP_F_VX * n + i] = S.f[SF_VX * p + i]; f64[SALP_F_VY * n + i] = S.f[SF_VY * p + i];
    f64[SALP_F_THETA * n + i] = S.f[SF_TH * p + i]; f64[SALP_F_OMEGA * n + i] = S.f[SF_OM * p + i];
    f64[SALP_F_NOZZLE * n + i] = S.f[SF_NOZ * p + i];
    const double water = S.f[SF_WATER * p + i];
    f64[SALP_F_WATER * n + i] = water;
    double a, b;
    shape_of<false>(P, packed, water, a, b);
    f64[SALP_F_ELLIPSE_A * n + i] = a; f64[SALP_F_ELLIPSE_B * n + i] = b;
    for (int k = 0; k < 2 * P.F; ++k) f64[(SALP_F_FOOD0 + k) * n + i] = S.f[(SF_FOOD0 + k) * p + i];
  }
  if (i32) {
    i32[SALP_I_PHASE * n + i] = bw_phase(packed); i32[SALP_I_TIMER * n + i] = bw_timer(packed);
    i32[SALP_I_EXHALE_DUR * n + i] = bw_dur(packed); i32[SALP_I_SHAPE_HOLD * n + i] = bw_hold(packed);
    i32[SALP_I_STEPS_SINCE_FOOD * n + i] = S.i[SI_SSF * p + i];
    i32[SALP_I_FOOD_COLLECTED * n + i] = S.i[SI_FC * p + i];
    i32[SALP_I_RNG_COUNTER * n + i] = S.i[SI_RNG * p + i];
    i32[SALP_I_EPISODE_LENGTH * n + i] = S.i[SI_EPLEN * p + i];
  }
}

__global__ void salp_set_state_kernel(DevParams P, DevState S, const double* f64, const int32_t* i32) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.n) return;
  const int64_t p = P.pitch, n = P.n;
  if (f64) {
    S.f[SF_X * p + i] = f64[SALP_F_X * n + i]; S.f[SF_Y * p + i] = f64[SALP_F_Y * n + i];
    S.f[SF_VX * p + i] = f64[SALP_F_VX * n + i]; S.f[SF_VY * p + i] = f64[SALP_F_VY * n + i];
    S.f[SF_TH * p + i] = f64[SALP_F_THETA * n + i]; S.f[SF_OM * p + i] = f64[SALP_F_OMEGA * n + i];
    S.f[SF_NOZ * p + i] = f64[SALP_F_NOZZLE * n + i]; S.f[SF_WATER * p + i] = f64[SALP_F_WATER * n + i];
    for (int k = 0; k < P.F; ++k) {
      double fx = f64[(SALP_F_FOOD0 + k) * n + i], fy = f64[(SALP_F_FOOD0 + P.F + k) * n + i];
      if (fx != fx || fy != fy) { fx = __builtin_nan(""); fy = __builtin_nan(""); }
      S.f[(SF_FOOD0 + k) * p + i] = fx; S.f[(SF_FOOD0 + P.F + k) * p + i] = fy;
    }
  }
  if (i32) {
    S.i[SI_PACKED * p + i] = (int32_t)pack_breath(i32[SALP_I_PHASE * n + i], i32[SALP_I_TIMER * n + i],
                                                  i32[SALP_I_EXHALE_DUR * n + i], i32[SALP_I_SHAPE_HOLD * n + i]);
    S.i[SI_SSF * p + i] = i32[SALP_I_STEPS_SINCE_FOOD * n + i];
    S.i[SI_FC * p + i] = i32[SALP_I_FOOD_COLLECTED * n + i];
    S.i[SI_RNG * p + i] = i32[SALP_I_RNG_COUNTER * n + i];
    S.i[SI_EPLEN * p + i] = i32[SALP_I_EPISODE_LENGTH * n + i];
  }
}

// salp_vec_reseed: the state a freshly created handle has before its initial reset (every row zero, draw counters
// included), the new key words, cleared statistics.  The reset kernel that follows on the same stream reads the new key.
__global__ __launch_bounds__(kBlock) void salp_reseed_kernel(ColdBlock* cold, DevStats* stats, int64_t pitch, int nf_rows,
                                                            uint32_t seed_lo, uint32_t seed_hi) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < pitch) {
    double* f = cold->S.f;
    int32_t* w = cold->S.i;
    for (int r = 0; r < nf_rows; ++r) f[(int64_t)r * pitch + i] = 0.0;
    for (int r = 0; r < SI_COUNT; ++r) w[(int64_t)r * pitch + i] = 0;
  }
  if (i == 0) { cold->seed[0] = seed_lo; cold->seed[1] = seed_hi; }
  if (i < (int64_t)SALP_STATS_REPLICAS * 16) stats[i / 16].v[i % 16] = 0ull;
}

// public layout -> device block of P policies (salp_policy.h): one thread per word of the block
__global__ __launch_bounds__(kBlock) void salp_policy_relayout_kernel(float* __restrict__ block, const float* __restrict__ pub,
                                                                      const int32_t* __restrict__ map, int stride, int words, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  const int64_t p = i / stride;
  const int m = map[i - p * stride];
  block[PH_WORDS + i] = m >= 0 ? pub[p * words + m] : 0.f;
}

// The policy's noise step (header words PH_NOISE, PH_NOISE + 1 of its device block): one thread, behind the launches that read it
__global__ void salp_policy_noise_kernel(float* block, uint64_t add, uint64_t set, int do_set) {
  uint32_t* const w = reinterpret_cast<uint32_t*>(block) + PH_NOISE;
  const uint64_t v = do_set ? set : ((((uint64_t)w[1] << 32) | w[0]) + add);
  w[0] = (uint32_t)v;
  w[1] = (uint32_t)(v >> 32);
}

// ---- test support: the snake step's math primitives on their own (salp_snake_math_probe, salp_snake_math_probe.h) ----
// Element i on thread i; `function` is uniform, so the table pointer and the key words stay scalar as in the step.
template <bool STD>
__device__ __forceinline__ void probe_thrust_terms(const DevParams& P, const double* in, double* out, int64_t n, int64_t i) {
  const uint64_t genv = (uint64_t)(uint32_t)in[5 * n + i] | ((uint64_t)(uint32_t)in[6 * n + i] << 32);
  const ThrustTerms t = jet_thrust_terms<STD>(in[i], in[n + i], in[2 * n + i], in[3 * n + i], (uint32_t)in[4 * n + i], genv, P);
  out[i] = t.ax; out[n + i] = t.ay; out[2 * n + i] = t.bx; out[3 * n + i] = t.by;
  out[4 * n + i] = t.cx; out[5 * n + i] = t.cy; out[6 * n + i] = t.om;
}
__global__ __launch_bounds__(kBlock) void salp_snake_math_probe_kernel(DevParams P, int function, const double* in, double* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  switch (function) {
    case SALP_SNAKE_MATH_SINCOS_T: { double s, c; sincos_small_t(thrust_table(), in[i], s, c); out[i] = s; out[n + i] = c; break; }
    case SALP_SNAKE_MATH_SIN_NOZZLE_T: out[i] = sin_nozzle_t(thrust_table(), in[i]); break;
    case SALP_SNAKE_MATH_ATAN2: out[i] = (double)atan2_fast<false>((float)in[i], (float)in[n + i]); break;
    case SALP_SNAKE_MATH_ATAN2_PRECISE: out[i] = (double)atan2_fast<true>((float)in[i], (float)in[n + i]); break;
    case SALP_SNAKE_MATH_COS_WRAPPED: out[i] = (double)cos_wrapped((float)in[i]); break;
    case SALP_SNAKE_MATH_REL_HEADING:
      out[i] = (double)relative_heading<false>((float)in[i], (float)in[n + i], (float)in[2 * n + i]);
      break;
    case SALP_SNAKE_MATH_REL_HEADING_PRECISE:
      out[i] = (double)relative_heading<true>((float)in[i], (float)in[n + i], (float)in[2 * n + i]);
      break;
    case SALP_SNAKE_MATH_PHILOX: {
      const U4 w = philox4x32_10((uint32_t)in[i], (uint32_t)in[n + i], (uint32_t)in[2 * n + i], (uint32_t)in[3 * n + i],
                                 (uint32_t)in[4 * n + i], (uint32_t)in[5 * n + i]);
      out[i] = (double)w.x; out[n + i] = (double)w.y; out[2 * n + i] = (double)w.z; out[3 * n + i] = (double)w.w;
      break;
    }
    case SALP_SNAKE_MATH_U53: out[i] = u53((uint32_t)in[i], (uint32_t)in[n + i]); break;
    case SALP_SNAKE_MATH_THRUST_STD: probe_thrust_terms<true>(P, in, out, n, i); break;
    case SALP_SNAKE_MATH_THRUST_RT: probe_thrust_terms<false>(P, in, out, n, i); break;
    default: break;
  }
}

}  // namespace
