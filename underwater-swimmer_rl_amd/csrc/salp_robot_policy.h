// salp_robot_policy.h — the in-kernel MLP policy of salp_robot_vec_rollout_policy: the deterministic policy of
// include/salp_vec.h "Policy" for the robot's 6 observations and 3 action components.  Device code only; the host side
// (check_policy_desc, policy_block_map, policy_header) and the block layout are those of salp_policy.h, which are generic in
// the dimensions: with obs_dim 6 a hidden chunk of the first layer is 16 (6 + 1) words, the tail holds b_last[3], scale[3],
// shift[3] in its first nine words, and a last-layer row without hidden layers is padded from 6 to 16 words.
//
// The arithmetic is the fixed order stated in salp_policy.h: fp32; every unit starts from its bias and adds its inputs in
// index order with one fmaf each; relu; tanhf or the clamp to [-1, 1]; one multiply by scale, one add of shift.  The
// functions here follow policy_eval_impl of salp_policy.h piece by piece (which stays as it is: the snake rollout kernels
// are compiled from it) with three action sums instead of two.
//
// SAMPLED (salp_robot_vec_rollout_policy_sampled, include/salp_robot_sampled.h): the tanh-Gaussian sample of
// include/salp_vec.h "Sampled actions" with three components.  The log-std tail and rows sit behind the mean head where
// policy_block_map(6, 3, d, true, ...) puts them (row stride 16 words without a hidden layer, else the last hidden width);
// the head's sums ride in the fused chunk loop like the mean head's, so both keep index order.  The deterministic
// instantiation is the function it was before the sampled form existed: everything new sits behind `if constexpr`.
#pragma once
#include "salp_policy.h"

namespace salp {

#ifdef __HIPCC__
enum { ROBOT_POLICY_OBS = 6, ROBOT_POLICY_ACT = 3 };

// u[a] += sum_j W_last[a][16 c + j] v[j]: the last layer's share of one chunk of its input
template <int AD>
__device__ __forceinline__ void robot_policy_last_chunk(pol_float* wl, int row_stride, int c, const float (&v)[POLICY_CHUNK], float (&u)[AD]) {
#pragma unroll
  for (int a = 0; a < AD; ++a) {
    const pol_v16 w = pol_load16(wl + a * row_stride + POLICY_CHUNK * c);
#pragma unroll
    for (int j = 0; j < POLICY_CHUNK; ++j) u[a] = __builtin_fmaf(w[j], v[j], u[a]);
  }
}

// The action of one env from its observation row `x`.  `blk`: the device block; `pol_off`: word offset of this wavefront's
// policy behind the header (wave-uniform).  Called under the EXEC mask of the lanes that start a cycle: the scalar loads
// serve whichever lanes are on.
// SAMPLED: z[a] is the standard normal draw of component a; `logp` receives the log-probability of the sampled action.
template <int OD, int AD, bool SAMPLED>
__device__ __forceinline__ void robot_policy_eval_impl(const float* blk, uint32_t pol_off, const float (&x)[OD], float (&act)[AD],
                                                       [[maybe_unused]] const float (&z)[AD], [[maybe_unused]] float& logp) {
  static_assert(OD <= POLICY_CHUNK && 3 * AD <= POLICY_TAIL_WORDS, "one padded last-layer row, one tail group");
  const uint64_t adr = (uint64_t)(uintptr_t)blk;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)adr);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(adr >> 32));
  pol_int* hd = (pol_int*)(uintptr_t)(((uint64_t)hi << 32) | lo);
  asm volatile("" : "+s"(hd));
  const int nh = hd[PH_NHIDDEN], h0 = hd[PH_H0], h1 = hd[PH_H1], out_act = hd[PH_OUT];
  pol_float* w = (pol_float*)hd + PH_WORDS + (uint32_t)__builtin_amdgcn_readfirstlane((int)pol_off);

  const int c0n = h0 / POLICY_CHUNK, c1n = h1 / POLICY_CHUNK;
  const int l0_words = c0n * POLICY_CHUNK * (OD + 1);
  const int l1_words = c1n * POLICY_CHUNK * (h0 + 1);
  pol_float* tail = w + (nh >= 1 ? l0_words : 0) + (nh >= 2 ? l1_words : 0);
  pol_float* wl = tail + POLICY_TAIL_WORDS;
  const pol_v16 tl = pol_load16(tail);      // b_last[AD], scale[AD], shift[AD]
  float u[AD];
#pragma unroll
  for (int a = 0; a < AD; ++a) u[a] = tl[a];
  [[maybe_unused]] float ls[AD];            // SAMPLED: the log-std head's sums
  [[maybe_unused]] pol_float* wl2 = wl;
  if constexpr (SAMPLED) {
    const int rs = nh == 0 ? POLICY_CHUNK : (nh == 1 ? h0 : h1);      // row stride of the last layer
    pol_float* tail2 = wl + AD * rs;
    wl2 = tail2 + POLICY_TAIL_WORDS;
    const pol_v16 t2 = pol_load16(tail2);   // b_ls[AD]
#pragma unroll
    for (int a = 0; a < AD; ++a) ls[a] = t2[a];
  }

  if (nh == 0) {
#pragma unroll
    for (int a = 0; a < AD; ++a) {
      const pol_v16 wa = pol_load16(wl + a * POLICY_CHUNK);     // the row's OD words, zero-padded to 16
#pragma unroll
      for (int i = 0; i < OD; ++i) u[a] = __builtin_fmaf(wa[i], x[i], u[a]);
    }
    if constexpr (SAMPLED) {
#pragma unroll
      for (int a = 0; a < AD; ++a) {
        const pol_v16 wa = pol_load16(wl2 + a * POLICY_CHUNK);
#pragma unroll
        for (int i = 0; i < OD; ++i) ls[a] = __builtin_fmaf(wa[i], x[i], ls[a]);
      }
    }
  } else if (nh == 1) {
#pragma unroll 1
    for (int c = 0; c < c0n; ++c) {
      float acc[POLICY_CHUNK];
      policy_chunk_regs<OD>(w + c * (POLICY_CHUNK * (OD + 1)), x, acc);
#pragma unroll
      for (int j = 0; j < POLICY_CHUNK; ++j) acc[j] = fmaxf(acc[j], 0.f);
      robot_policy_last_chunk<AD>(wl, h0, c, acc, u);
      if constexpr (SAMPLED) robot_policy_last_chunk<AD>(wl2, h0, c, acc, ls);
    }
  } else {
    float h[POLICY_MAX_HIDDEN];
#pragma unroll
    for (int g = 0; g < POLICY_MAX_HIDDEN / POLICY_CHUNK; ++g) {
      if (g < c0n) {
        float acc[POLICY_CHUNK];
        policy_chunk_regs<OD>(w + g * (POLICY_CHUNK * (OD + 1)), x, acc);
#pragma unroll
        for (int j = 0; j < POLICY_CHUNK; ++j) h[POLICY_CHUNK * g + j] = fmaxf(acc[j], 0.f);
      } else {
#pragma unroll
        for (int j = 0; j < POLICY_CHUNK; ++j) h[POLICY_CHUNK * g + j] = 0.f;
      }
    }
    pol_float* w1 = w + l0_words;
    const int chunk_words = POLICY_CHUNK * (h0 + 1);
#pragma unroll 1
    for (int c = 0; c < c1n; ++c) {
      pol_float* wc = w1 + c * chunk_words;
      float acc[POLICY_CHUNK];
      const pol_v16 b = pol_load16(wc);
#pragma unroll
      for (int j = 0; j < POLICY_CHUNK; ++j) acc[j] = b[j];
#pragma unroll
      for (int g = 0; g < POLICY_MAX_HIDDEN / POLICY_CHUNK; ++g) {
        if (g < c0n) {
#pragma unroll
          for (int ii = 0; ii < POLICY_CHUNK; ++ii) {
            const int i = POLICY_CHUNK * g + ii;
            const pol_v16 wv = pol_load16(wc + POLICY_CHUNK * (1 + i));
#pragma unroll
            for (int j = 0; j < POLICY_CHUNK; ++j) acc[j] = __builtin_fmaf(wv[j], h[i], acc[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < POLICY_CHUNK; ++j) acc[j] = fmaxf(acc[j], 0.f);
      robot_policy_last_chunk<AD>(wl, h1, c, acc, u);
      if constexpr (SAMPLED) robot_policy_last_chunk<AD>(wl2, h1, c, acc, ls);
    }
  }
  if constexpr (SAMPLED) {
    // a Gaussian policy's output activation is tanh (salp_robot_policy_create_gaussian); the log-probability's terms are
    // added in component order, each a fixed sequence of fp32 roundings (include/salp_vec.h "Sampled actions")
    float lp = 0.f;
#pragma unroll
    for (int a = 0; a < AD; ++a) {
      const float l = fminf(fmaxf(ls[a], -20.0f), 2.0f);
      const float sd = expf(l);
      const float s = __builtin_fmaf(sd, z[a], u[a]);
      const float m2 = -2.0f * s;
      const float sp = fmaxf(m2, 0.f) + log1pf(expf(-fabsf(m2)));
      const float c = (0.693147180559945309f - s) - sp;
      float g = -0.5f * (z[a] * z[a]);
      g = g - l;
      g = g - 0.918938533204672742f;
      g = g - 2.0f * c;
      lp = lp + g;
      act[a] = tanhf(s) * tl[AD + a] + tl[2 * AD + a];
    }
    logp = lp;
  } else {
#pragma unroll
    for (int a = 0; a < AD; ++a) {
      const float v = out_act ? fminf(fmaxf(u[a], -1.0f), 1.0f) : tanhf(u[a]);
      act[a] = v * tl[AD + a] + tl[2 * AD + a];
    }
  }
}

template <int OD, int AD>
__device__ __forceinline__ void robot_policy_eval(const float* blk, uint32_t pol_off, const float (&x)[OD], float (&act)[AD]) {
  const float z[AD] = {};
  float unused = 0.f;
  robot_policy_eval_impl<OD, AD, false>(blk, pol_off, x, act, z, unused);
}

// The sampled action and its log-probability from the draws z (one per component)
template <int OD, int AD>
__device__ __forceinline__ void robot_policy_eval_sampled(const float* blk, uint32_t pol_off, const float (&x)[OD],
                                                          const float (&z)[AD], float (&act)[AD], float& logp) {
  robot_policy_eval_impl<OD, AD, true>(blk, pol_off, x, act, z, logp);
}
#endif  // __HIPCC__

}  // namespace salp
