// salp_policy.h — the in-kernel MLP policy of salp_vec_rollout_policy and salp_robot_vec_rollout_policy (include/salp_vec.h
// "Policy"): the device block's layout, shared by the host (which builds it) and the rollout kernels (which evaluate it:
// the snake's once per env-step, the robot's once per breathing cycle), and the one evaluation function of both.  Two
// shapes run: the snake's 24 observations and 1 or 2 action components, the robot's 6 and 3.
//
// Device block, 32-bit words:  [PH_WORDS header][policy 0][policy 1]...  each policy `stride` words, a multiple of 16, so
// that every 16-word group below starts on a 64-byte boundary.  One policy (IN = obs_dim for the first layer, else the
// width of the layer before):
//   per hidden layer, per chunk c of 16 output units:   b[16 c .. 16 c + 15], then for i = 0 .. IN-1 the 16 weights
//                                                        W[16 c + j][i], j = 0 .. 15        (16 (IN + 1) words per chunk:
//                                                        16 (obs_dim + 1) in the first layer, 400 or 112 words)
//   tail (16 words):                                     b_last[A], scale[A], shift[A] in its first 3 A words (3, 6 or 9),
//                                                        zero padding
//   last layer, per action a:                            W_last[a][0 .. IN-1], zero-padded to a multiple of 16 words
//                                                        (without a hidden layer: 24 -> 32, 6 -> 16)
// A Gaussian policy (salp_policy_create_gaussian; header word PH_GAUSS then holds the value 1 — a mark for whoever inspects a block,
// no kernel reads it: the host decides from its own record which kernels a policy may run) carries its log-std head behind that, in the
// same form:
//   log-std tail (16 words):                             b_ls[A], zero padding
//   log-std head, per action a:                          W_ls[a][0 .. IN-1], zero-padded to a multiple of 16 words
// so the block of its mean policy is a prefix of each policy's words and the deterministic evaluation never reads the rest.
// Header words PH_NOISE, PH_NOISE + 1: the policy's 64-bit noise step (include/salp_vec.h "Randomness"), read by the
// sampling kernels at entry and advanced by a one-thread kernel behind them.
// The weights are wave-uniform (a wavefront never mixes policies), so everything is read through the constant address
// space with scalar loads (s_load_dwordx16: one load feeds 16 v_fmac with a scalar operand each); the base is made opaque
// inside policy_eval so that the loads stay in the function instead of being hoisted across the step loop.
//
// Arithmetic (fixed, the same in every instantiation): fp32; every unit starts from its bias and adds its inputs in index
// order with one fmaf each; relu = fmaxf(., 0); tanhf or a clamp to [-1, 1]; then one multiply by scale and one add of
// shift (two roundings).  The last layer is fused into the chunk loop of the layer before it — chunks and their units
// are visited in index order, so its sum keeps the same order (the log-std head of a sampling evaluation rides along in the
// same way) — and the only activations that are stored are those of
// the FIRST of two hidden layers: at most 64 VGPRs (indexed at compile time; the widths are run-time values tested per
// group of 16, wave-uniform).
//
// The header has a host section and a device section.  The host section — the descriptor's ranges, the map from the public
// layout (include/salp_vec.h) to the block above, the header words and the allocations' byte counts — is plain C++17 with no HIP call and no fail(), like
// the host functions of salp_params.h: tests/policy_host.cpp compiles it with g++, so the layout is under test without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/salp_vec.h"   // salp_policy_desc_t, SALP_POLICY_OUT_*, SALP_OK, SALP_ERR_INVALID

namespace salp {

enum { PH_NHIDDEN = 0, PH_H0, PH_H1, PH_OUT, PH_STRIDE, PH_GROUP, PH_COUNT, PH_GAUSS, PH_NOISE = 8 /* two words, lo then hi */, PH_WORDS = 16 };
enum { POLICY_CHUNK = 16, POLICY_MAX_HIDDEN = 64, POLICY_TAIL_WORDS = 16 };
enum { POLICY_WAVE = 64 };   // envs of one wavefront (kWave of the kernels)

// ------------------------------------------------------------------ host side: descriptor -> ranges, block map, header
// A wavefront never mixes policies: P policies share the envs in equal runs of whole wavefronts.
inline int check_n_policies(int64_t n_envs, int P, const char** why) {
  if (P > 1 && (n_envs % P != 0 || (n_envs / P) % POLICY_WAVE != 0)) {
    *why = "n_policies > 1 needs n_envs % P == 0 and (n_envs / P) % 64 == 0";
    return (int)SALP_ERR_INVALID;
  }
  return (int)SALP_OK;
}

// The descriptor's ranges (include/salp_vec.h) for a handle of these dimensions.  SALP_OK with *words (nullable) = public
// words of one policy, or SALP_ERR_INVALID with the reason in *why.
inline int check_policy_desc(int obs_dim, int act_dim, int kmax, int64_t n_envs, const salp_policy_desc_t* d, bool gaussian,
                             int* words, const char** why) {
  const auto refuse = [why](const char* msg) { *why = msg; return (int)SALP_ERR_INVALID; };
  if (!d) return refuse("handle/desc is NULL");
  if (d->struct_size != sizeof(salp_policy_desc_t)) return refuse("salp_policy_desc_t.struct_size mismatch");
  if (kmax != 3) return refuse("policies need a handle with max_observed_food == 3");
  if (d->n_hidden < 0 || d->n_hidden > 2) return refuse("n_hidden must be 0, 1 or 2");
  for (int l = 0; l < 2; ++l) {
    const int w = d->hidden[l];
    if (l < d->n_hidden ? (w < POLICY_CHUNK || w > POLICY_MAX_HIDDEN || w % POLICY_CHUNK) : (w != 0))
      return refuse("hidden widths must be multiples of 16 in [16, 64] (unused entries 0)");
  }
  if (d->out_activation != SALP_POLICY_OUT_TANH && d->out_activation != SALP_POLICY_OUT_CLIP)
    return refuse("out_activation must be SALP_POLICY_OUT_TANH or SALP_POLICY_OUT_CLIP");
  if (gaussian && d->out_activation != SALP_POLICY_OUT_TANH)
    return refuse("a Gaussian policy's out_activation must be SALP_POLICY_OUT_TANH");
  if (d->n_policies < 1) return refuse("n_policies must be >= 1");
  if (const int rc = check_n_policies(n_envs, d->n_policies, why)) return rc;
  int in = obs_dim, w = 0;
  for (int l = 0; l < d->n_hidden; ++l) { w += d->hidden[l] * in + d->hidden[l]; in = d->hidden[l]; }
  w += act_dim * in + 3 * act_dim;
  if (gaussian) w += act_dim * in + act_dim;     // the log-std head
  if (words) *words = w;
  return (int)SALP_OK;
}

// map[k] = the public word that word k of a policy in the device block holds, -1 = zero (the layout above for the block,
// include/salp_vec.h for the public layout); `d` has passed check_policy_desc.  Returns the stride: every piece is a
// multiple of 16 words.
inline int policy_block_map(int obs_dim, int act_dim, const salp_policy_desc_t& d, bool gaussian, std::vector<int32_t>& map) {
  map.clear();
  const auto push = [&map](int32_t v) { map.push_back(v); };
  const int AD = act_dim;
  int in = obs_dim, pubo = 0;
  for (int l = 0; l < d.n_hidden; ++l) {
    const int O = d.hidden[l], Wp = pubo, bp = pubo + O * in;
    for (int c = 0; c < O / POLICY_CHUNK; ++c) {
      for (int j = 0; j < POLICY_CHUNK; ++j) push(bp + c * POLICY_CHUNK + j);
      for (int i = 0; i < in; ++i)
        for (int j = 0; j < POLICY_CHUNK; ++j) push(Wp + (c * POLICY_CHUNK + j) * in + i);
    }
    pubo = bp + O; in = O;
  }
  // Gaussian: W_mu, b_mu, W_ls, b_ls, scale, shift in the public layout; the log-std head behind the mean head in the block
  const int Wl = pubo, bl = pubo + AD * in, W2 = bl + AD, b2 = W2 + AD * in, sc = gaussian ? b2 + AD : bl + AD, sh = sc + AD;
  for (int k = 0; k < POLICY_TAIL_WORDS; ++k) push(k < AD ? bl + k : (k < 2 * AD ? sc + k - AD : (k < 3 * AD ? sh + k - 2 * AD : -1)));
  const int rs = (in + POLICY_CHUNK - 1) / POLICY_CHUNK * POLICY_CHUNK;    // 24 -> 32 for the linear policy
  for (int a = 0; a < AD; ++a)
    for (int i = 0; i < rs; ++i) push(i < in ? Wl + a * in + i : -1);
  if (gaussian) {
    for (int k = 0; k < POLICY_TAIL_WORDS; ++k) push(k < AD ? b2 + k : -1);
    for (int a = 0; a < AD; ++a)
      for (int i = 0; i < rs; ++i) push(i < in ? W2 + a * in + i : -1);
  }
  return (int)map.size();
}

// The PH_WORDS header words of a block of d.n_policies policies of `stride` words each, bound to a handle of n_envs envs.
inline void policy_header(const salp_policy_desc_t& d, int stride, int64_t n_envs, bool gaussian, int32_t (&hd)[PH_WORDS]) {
  for (int32_t& w : hd) w = 0;     // (noise step: 0)
  hd[PH_NHIDDEN] = d.n_hidden; hd[PH_H0] = d.hidden[0]; hd[PH_H1] = d.hidden[1]; hd[PH_OUT] = d.out_activation;
  hd[PH_STRIDE] = stride; hd[PH_COUNT] = d.n_policies; hd[PH_GAUSS] = gaussian ? 1 : 0;
  hd[PH_GROUP] = d.n_policies > 1 ? (int32_t)(n_envs / d.n_policies) : 0x7FFFFFFF;
}

// The byte counts of a policy object's three device allocations: the block (header + d.n_policies policies of `stride`
// words), the staging of the public layout ([n_policies][words]) and the map ([stride]).
struct PolicyBytes { size_t block, pub, map; };
inline PolicyBytes policy_bytes(const salp_policy_desc_t& d, int words, int stride) {
  return {((size_t)PH_WORDS + (size_t)d.n_policies * stride) * sizeof(float), (size_t)d.n_policies * words * sizeof(float),
          (size_t)stride * sizeof(int32_t)};
}

// ------------------------------------------------------------------ device side
#ifdef __HIPCC__
typedef const float __attribute__((address_space(4))) pol_float;
typedef const int32_t __attribute__((address_space(4))) pol_int;
typedef float pol_v16 __attribute__((ext_vector_type(16)));
typedef float pol_v8 __attribute__((ext_vector_type(8)));
typedef const pol_v16 __attribute__((address_space(4))) pol_v16c;
typedef const pol_v8 __attribute__((address_space(4))) pol_v8c;

__device__ __forceinline__ pol_v16 pol_load16(pol_float* p) { return *reinterpret_cast<pol_v16c*>(p); }
__device__ __forceinline__ pol_v8 pol_load8(pol_float* p) { return *reinterpret_cast<pol_v8c*>(p); }

// acc[j] = b[j] + sum_i W[j][i] x[i] over the NIN register inputs, for the chunk whose block starts at `wc`
template <int NIN>
__device__ __forceinline__ void policy_chunk_regs(pol_float* wc, const float (&x)[NIN], float (&acc)[POLICY_CHUNK]) {
  const pol_v16 b = pol_load16(wc);
#pragma unroll
  for (int j = 0; j < POLICY_CHUNK; ++j) acc[j] = b[j];
#pragma unroll
  for (int i = 0; i < NIN; ++i) {
    const pol_v16 w = pol_load16(wc + POLICY_CHUNK * (1 + i));
#pragma unroll
    for (int j = 0; j < POLICY_CHUNK; ++j) acc[j] = __builtin_fmaf(w[j], x[i], acc[j]);
  }
}

// u[a] += sum_j W_last[a][16 c + j] relu'd[j]: the last layer's share of one chunk of its input
template <int AD>
__device__ __forceinline__ void policy_last_chunk(pol_float* wl, int row_stride, int c, const float (&v)[POLICY_CHUNK], float (&u)[AD]) {
#pragma unroll
  for (int a = 0; a < AD; ++a) {
    const pol_v16 w = pol_load16(wl + a * row_stride + POLICY_CHUNK * c);
#pragma unroll
    for (int j = 0; j < POLICY_CHUNK; ++j) u[a] = __builtin_fmaf(w[j], v[j], u[a]);
  }
}

// This block's header through scalar loads: the address, the same in every lane, moved to scalar registers and into the
// constant address space
__device__ __forceinline__ pol_int* policy_block_header(const float* blk) {
  const uint64_t adr = (uint64_t)(uintptr_t)blk;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)adr);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(adr >> 32));
  return (pol_int*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

// The tail's first 3 AD words (b_last, scale, shift; b_ls of the log-std tail) in the narrowest load that holds them
template <int AD>
__device__ __forceinline__ auto policy_load_tail(pol_float* p) {
  if constexpr (3 * AD <= 8) return pol_load8(p); else return pol_load16(p);
}

// u[a] += sum_i W_last[a][i] x[i]: the last layer of a policy without hidden layers.  A row is its OD words zero-padded to
// POLICY_ROW<OD>: one 16-word group, or 16 + 8 words of 32 for the snake's 24 observations
template <int OD> constexpr int POLICY_ROW = (OD + POLICY_CHUNK - 1) / POLICY_CHUNK * POLICY_CHUNK;
template <int OD, int AD>
__device__ __forceinline__ void policy_last_rows(pol_float* wl, const float (&x)[OD], float (&u)[AD]) {
#pragma unroll
  for (int a = 0; a < AD; ++a) {
    const pol_v16 wa = pol_load16(wl + a * POLICY_ROW<OD>);
    if constexpr (OD <= 16) {
#pragma unroll
      for (int i = 0; i < OD; ++i) u[a] = __builtin_fmaf(wa[i], x[i], u[a]);
    } else {
      const pol_v8 wb = pol_load8(wl + a * POLICY_ROW<OD> + 16);
#pragma unroll
      for (int i = 0; i < 16; ++i) u[a] = __builtin_fmaf(wa[i], x[i], u[a]);
#pragma unroll
      for (int i = 0; i < OD - 16; ++i) u[a] = __builtin_fmaf(wb[i], x[16 + i], u[a]);
    }
  }
}

// The action of one env from its observation row `x` (OD floats in registers).  `blk`: the device block; `pol_off`: word
// offset of this wavefront's policy behind the header (wave-uniform).  The scalar loads serve whichever lanes are on.
// SAMPLED: the tanh-Gaussian sample of include/salp_vec.h "Sampled actions" from the standard normal draws z[a]; `logp`
// receives its log-probability.  The mean's arithmetic is that of the deterministic evaluation, unit by unit.
template <int OD, int AD, bool SAMPLED>
__device__ __forceinline__ void policy_eval_impl(const float* blk, uint32_t pol_off, const float (&x)[OD], float (&act)[AD],
                                                 [[maybe_unused]] const float (&z)[AD], [[maybe_unused]] float& logp) {
  static_assert(OD == 24 || OD <= POLICY_CHUNK, "a last-layer row without hidden layers is read as 16 + 8 words (24 observations) or as one 16-word group");
  static_assert(OD != 24 || AD <= 2, "24 observations are the snake's (max_observed_food == 3): 1 or 2 action components");
  static_assert(3 * AD <= POLICY_TAIL_WORDS, "b_last, scale and shift share the tail's one 16-word group");
  pol_int* hd = policy_block_header(blk);
  asm volatile("" : "+s"(hd));
  const int nh = hd[PH_NHIDDEN], h0 = hd[PH_H0], h1 = hd[PH_H1], out_act = hd[PH_OUT];
  pol_float* w = (pol_float*)hd + PH_WORDS + (uint32_t)__builtin_amdgcn_readfirstlane((int)pol_off);

  const int c0n = h0 / POLICY_CHUNK, c1n = h1 / POLICY_CHUNK;
  const int l0_words = c0n * POLICY_CHUNK * (OD + 1);
  const int l1_words = c1n * POLICY_CHUNK * (h0 + 1);
  pol_float* tail = w + (nh >= 1 ? l0_words : 0) + (nh >= 2 ? l1_words : 0);
  pol_float* wl = tail + POLICY_TAIL_WORDS;
  const auto tl = policy_load_tail<AD>(tail);      // b_last[AD], scale[AD], shift[AD]
  float u[AD];
#pragma unroll
  for (int a = 0; a < AD; ++a) u[a] = tl[a];
  [[maybe_unused]] float ls[AD];                   // SAMPLED: the log-std head's sums
  [[maybe_unused]] pol_float* wl2 = wl;
  if constexpr (SAMPLED) {
    const int rs = nh == 0 ? POLICY_ROW<OD> : (nh == 1 ? h0 : h1);      // row stride of the last layer
    pol_float* tail2 = wl + AD * rs;
    wl2 = tail2 + POLICY_TAIL_WORDS;
    const auto t2 = policy_load_tail<AD>(tail2);   // b_ls[AD]
#pragma unroll
    for (int a = 0; a < AD; ++a) ls[a] = t2[a];
  }

  if (nh == 0) {
    policy_last_rows<OD, AD>(wl, x, u);
    if constexpr (SAMPLED) policy_last_rows<OD, AD>(wl2, x, ls);
  } else if (nh == 1) {
#pragma unroll 1
    for (int c = 0; c < c0n; ++c) {
      float acc[POLICY_CHUNK];
      policy_chunk_regs<OD>(w + c * (POLICY_CHUNK * (OD + 1)), x, acc);
#pragma unroll
      for (int j = 0; j < POLICY_CHUNK; ++j) acc[j] = fmaxf(acc[j], 0.f);
      policy_last_chunk<AD>(wl, h0, c, acc, u);
      if constexpr (SAMPLED) policy_last_chunk<AD>(wl2, h0, c, acc, ls);
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
      policy_last_chunk<AD>(wl, h1, c, acc, u);
      if constexpr (SAMPLED) policy_last_chunk<AD>(wl2, h1, c, acc, ls);
    }
  }
  // How the results are passed: the snake's are formed in u[] and copied out, the robot's go to act[] as they are formed.
  // Each kernel's machine code changes when it is written the other one's way (profiles/robot_rollout_notes.md).
  float (&r)[AD] = OD == 24 ? u : act;
  if constexpr (SAMPLED) {
    // a Gaussian policy's output activation is tanh (salp_policy_create_gaussian); the log-probability's terms are added
    // in component order, each a fixed sequence of fp32 roundings (include/salp_vec.h "Sampled actions")
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
      r[a] = tanhf(s) * tl[AD + a] + tl[2 * AD + a];
    }
    logp = lp;
  } else {
#pragma unroll
    for (int a = 0; a < AD; ++a) {
      const float v = out_act ? fminf(fmaxf(u[a], -1.0f), 1.0f) : tanhf(u[a]);
      r[a] = v * tl[AD + a] + tl[2 * AD + a];
    }
  }
  if constexpr (OD == 24) {
#pragma unroll
    for (int a = 0; a < AD; ++a) act[a] = u[a];
  }
}

template <int OD, int AD>
__device__ __forceinline__ void policy_eval(const float* blk, uint32_t pol_off, const float (&x)[OD], float (&act)[AD]) {
  const float z[AD] = {};
  float unused = 0.f;
  policy_eval_impl<OD, AD, false>(blk, pol_off, x, act, z, unused);
}

// The sampled action and its log-probability from the draws z (one per component)
template <int OD, int AD>
__device__ __forceinline__ void policy_eval_sampled(const float* blk, uint32_t pol_off, const float (&x)[OD], const float (&z)[AD],
                                                    float (&act)[AD], float& logp) {
  policy_eval_impl<OD, AD, true>(blk, pol_off, x, act, z, logp);
}

// One standard normal draw from two words of the policy's noise block (include/salp_vec.h "Randomness"): Box-Muller on
// u1 in (0, 1], u2 in [0, 1), 24 bits each
__device__ __forceinline__ float policy_normal(uint32_t wa, uint32_t wb) {
  const float u1 = (float)((wa >> 8) + 1u) * 5.9604644775390625e-8f;
  const float u2 = (float)(wb >> 8) * 5.9604644775390625e-8f;
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}
#endif  // __HIPCC__

}  // namespace salp
