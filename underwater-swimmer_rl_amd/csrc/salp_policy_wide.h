// salp_policy_wide.h — the WIDE evaluation scheme of the in-kernel policy: actors of 1 or 2 hidden layers, each a multiple
// of 32 units up to 256, evaluated on the matrix cores (v_mfma_f32_32x32x2_f32) inside the one-food rollout kernels.  The
// scheme of salp_policy.h keeps one env per lane and feeds the weights as scalar operands; it stops at 64 units (64
// activation registers per lane).  Here a wavefront evaluates the MLP of its 64 envs as a sequence of 32 x 32 x 2 products:
// units are rows, envs are columns, the weights are the A operand, the activations the B operand; a 32 x 32 tile covers 32
// envs, so the wavefront works on its two env halves one after the other (the weights are read twice, and only the first
// hidden layer of ONE half is stored: 128 registers at 256 units).
//
// Arithmetic: that of salp_policy.h, bit for bit.  The fp32-input MFMA is a k-ordered fmaf chain (one rounding per product,
// no wider accumulation, subnormals kept), the accumulators start from the bias, and every B operand below holds inputs
// 2 s and 2 s + 1 in k-step s, so each unit's sum is: bias, then its inputs in ascending index order, one fma each.  For a
// width both schemes accept the two give identical bits.  From the two heads on (clamp, expf, the log-probability's terms,
// tanhf or the clamp, one multiply, one add) the tail restates policy_eval_impl's operations in its order.
//
// Operand maps of v_mfma_f32_32x32x2_f32 (lane l of 64):   A: A[i = l & 31][k = l >> 5]    B: B[k = l >> 5][j = l & 31]
//   C/D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5), reg = 0 .. 15          (wide_cd_row)
// v_permlane32_swap(a, b) exchanges a's lanes 32 .. 63 with b's lanes 0 .. 31.  With one env per lane, swap(x[2 s], x[2 s + 1])
// leaves in the first register the k-step-s B operand of envs 0 .. 31 and in the second that of envs 32 .. 63.  A result
// tile holds on lane half h rows 4 h + (reg & 3) + 8 (reg >> 2); swap(reg 4 q, reg 4 q + 1) yields the B operands of k-steps
// 4 q (rows 8 q, 8 q + 1) and 4 q + 2 (rows 8 q + 4, 8 q + 5), swap(reg 4 q + 2, reg 4 q + 3) those of k-steps 4 q + 1 and 4 q + 3:
// eight swaps turn a tile of 32 units into the next layer's 16 k-steps in ascending order.
//
// Device block: the header of salp_policy.h (word PH_WIDE holds 1: a mark for whoever inspects a block, the host decides
// from its own record which kernels a policy runs) and per policy `stride` words:
//   per hidden layer (IN = 24, then the width before), per tile t of 32 units:
//       bias   32 words   word 16 h + reg = b[32 t + wide_cd_row(reg, 32 h)]: what lane half h loads into its accumulators
//       A      IN / 8 groups of 256 words: word 256 g + 4 l + k = W[32 t + (l & 31)][2 (4 g + k) + (l >> 5)] — lane l reads
//              its four successive k-steps with one 16-byte load, a wavefront's load is one contiguous 1-KB run
//   tail   16 words: [0 .. 3] the bias of the last layer's rows (row a < AD: mean component a; Gaussian: row AD + a: log-std
//              component a; else 0), [4 .. 4 + AD) scale, [6 .. 6 + AD) shift, zero padding — read with scalar loads
//   last   IN / 8 groups of 32 words: word 32 g + 4 (4 h + r) + k = row r of the last layer, input 2 (4 g + k) + h.  Lane l
//              reads slot (l >> 5, l & 3): rows 4 .. 31 of the last layer's accumulator tile repeat rows 0 .. 3 and are
//              never read (a row of a product depends on its own A row only).
//
// The calling condition of policy_eval_wide: wave-uniform control flow with all 64 lanes enabled (the rollout kernels
// compute on every lane, also on those whose stores are predicated off).  Each env is one column of every product, so
// whatever a lane past the range carries cannot reach another env.
//
// The header has a host section (plain C++17, no HIP call, compiled by tests/wide_policy_host.cpp) and a device section.
#pragma once
#include "salp_policy.h"

namespace salp {

enum { PH_WIDE = 10 };       // header word: 1 for a block of this layout
enum { WIDE_TILE = 32, WIDE_MAX_HIDDEN = 256, WIDE_OBS = 24, WIDE_ROWS = 4 /* rows of the last layer that exist */ };
enum { WIDE_TAIL_SCALE = 4, WIDE_TAIL_SHIFT = 6 };

// ------------------------------------------------------------------ the maps, shared by host and device
// row of a 32 x 32 result tile that accumulator register `reg` of lane `lane` holds (its column is lane & 31)
constexpr int wide_cd_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
// the (row / column, k) of the A and B operand element that lane `lane` supplies (k within the k-step: 0 or 1)
constexpr int wide_ab_index(int lane) { return lane & 31; }
constexpr int wide_ab_k(int lane) { return lane >> 5; }
// word offset, inside a tile's A area, of the 4 words (k-steps 4 g .. 4 g + 3) that lane `lane` loads for group g
constexpr int wide_a_word(int g, int lane) { return 256 * g + 4 * lane; }
// the same inside the last layer's area: slot (lane >> 5, lane & 3)
constexpr int wide_last_word(int g, int lane) { return 32 * g + 4 * (4 * (lane >> 5) + (lane & 3)); }
// word offset of lane half h's 16 bias words inside a tile
constexpr int wide_bias_word(int h) { return 16 * h; }
// words of one tile of a layer with IN inputs: the bias and IN / 8 groups
constexpr int wide_tile_words(int in) { return WIDE_TILE + (in / 8) * 256; }
// the k-step of the next layer that result register `reg` becomes after the eight swaps, and the lane half whose value it
// keeps in lanes 0 .. 31 of that operand (documentation of wide_relu_reorder; the host twin checks it against wide_cd_row)
constexpr int wide_reorder_kstep(int reg) { return 4 * (reg >> 2) + ((reg & 2) ? 1 : 0) + ((reg & 1) ? 2 : 0); }

// ------------------------------------------------------------------ host side
// The descriptor's ranges of the wide scheme for a handle of these dimensions (food_slots: the kernel class's slot count, 1
// for num_food_items <= 1).  As check_policy_desc: SALP_OK with *words (nullable), or SALP_ERR_INVALID and the reason.
inline int check_policy_desc_wide(int obs_dim, int act_dim, int kmax, int food_slots, int64_t n_envs, const salp_policy_desc_t* d,
                                  bool gaussian, int* words, const char** why) {
  const auto refuse = [why](const char* msg) { *why = msg; return (int)SALP_ERR_INVALID; };
  if (!d) return refuse("handle/desc is NULL");
  if (d->struct_size != sizeof(salp_policy_desc_t)) return refuse("salp_policy_desc_t.struct_size mismatch");
  if (kmax != 3) return refuse("policies need a handle with max_observed_food == 3");
  if (obs_dim != WIDE_OBS || act_dim < 1 || act_dim > 2) return refuse("wide policies exist for the snake env only (24 observations, 1 or 2 action components)");
  if (food_slots != 1) return refuse("wide policies need a handle with num_food_items <= 1 (the one-food kernels)");
  if (d->n_hidden < 1 || d->n_hidden > 2) return refuse("a wide policy's n_hidden must be 1 or 2");
  for (int l = 0; l < 2; ++l) {
    const int w = d->hidden[l];
    if (l < d->n_hidden ? (w < WIDE_TILE || w > WIDE_MAX_HIDDEN || w % WIDE_TILE) : (w != 0))
      return refuse("a wide policy's hidden widths must be multiples of 32 in [32, 256] (unused entries 0)");
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
  if (gaussian) w += act_dim * in + act_dim;
  if (words) *words = w;
  return (int)SALP_OK;
}

// map[k] = the public word (include/salp_vec.h) that word k of a policy in the device block holds, -1 = zero; `d` has passed
// check_policy_desc_wide.  Returns the stride.
inline int policy_block_map_wide(int act_dim, const salp_policy_desc_t& d, bool gaussian, std::vector<int32_t>& map) {
  map.clear();
  const auto push = [&map](int32_t v) { map.push_back(v); };
  const int AD = act_dim;
  int in = WIDE_OBS, pubo = 0;
  for (int l = 0; l < d.n_hidden; ++l) {
    const int O = d.hidden[l], Wp = pubo, bp = pubo + O * in;
    for (int t = 0; t < O / WIDE_TILE; ++t) {
      for (int h = 0; h < 2; ++h)
        for (int reg = 0; reg < 16; ++reg) push(bp + WIDE_TILE * t + wide_cd_row(reg, 32 * h));
      for (int g = 0; g < in / 8; ++g)
        for (int lane = 0; lane < POLICY_WAVE; ++lane)
          for (int k = 0; k < 4; ++k) push(Wp + (WIDE_TILE * t + wide_ab_index(lane)) * in + 2 * (4 * g + k) + wide_ab_k(lane));
    }
    pubo = bp + O; in = O;
  }
  const int Wl = pubo, bl = pubo + AD * in, W2 = bl + AD, b2 = W2 + AD * in, sc = gaussian ? b2 + AD : bl + AD, sh = sc + AD;
  const auto row_word = [&](int r, int i) { return r < AD ? Wl + r * in + i : ((gaussian && r < 2 * AD) ? W2 + (r - AD) * in + i : -1); };
  for (int k = 0; k < POLICY_TAIL_WORDS; ++k) {
    int v = -1;
    if (k < WIDE_ROWS) v = k < AD ? bl + k : ((gaussian && k < 2 * AD) ? b2 + k - AD : -1);
    else if (k >= WIDE_TAIL_SCALE && k < WIDE_TAIL_SCALE + AD) v = sc + k - WIDE_TAIL_SCALE;
    else if (k >= WIDE_TAIL_SHIFT && k < WIDE_TAIL_SHIFT + AD) v = sh + k - WIDE_TAIL_SHIFT;
    push(v);
  }
  for (int g = 0; g < in / 8; ++g)
    for (int h = 0; h < 2; ++h)
      for (int r = 0; r < WIDE_ROWS; ++r)
        for (int k = 0; k < 4; ++k) push(row_word(r, 2 * (4 * g + k) + h));
  return (int)map.size();
}

// The header words of a wide block: policy_header's, and the mark.
inline void policy_header_wide(const salp_policy_desc_t& d, int stride, int64_t n_envs, bool gaussian, int32_t (&hd)[PH_WORDS]) {
  policy_header(d, stride, n_envs, gaussian, hd);
  hd[PH_WIDE] = 1;
}

// One more than the largest word index of a policy that policy_eval_wide reads for this shape, from the kernel's own
// address arithmetic (the offsets below are the ones it forms; every load is 4 words but the bias's 16 and the tail's 8).
// It must not exceed the stride.
inline int policy_wide_read_end(const salp_policy_desc_t& d) {
  int end = 0, off = 0, in = WIDE_OBS;
  const auto reads = [&end](int first, int n) { if (first + n > end) end = first + n; };
  for (int l = 0; l < d.n_hidden; ++l) {
    for (int t = 0; t < d.hidden[l] / WIDE_TILE; ++t) {
      const int tile = off + t * wide_tile_words(in);
      for (int h = 0; h < 2; ++h) reads(tile + wide_bias_word(h), 16);
      for (int g = 0; g < in / 8; ++g)
        for (int lane = 0; lane < POLICY_WAVE; ++lane) reads(tile + WIDE_TILE + wide_a_word(g, lane), 4);
    }
    off += d.hidden[l] / WIDE_TILE * wide_tile_words(in);
    in = d.hidden[l];
  }
  reads(off, 8);
  off += POLICY_TAIL_WORDS;
  for (int g = 0; g < in / 8; ++g)
    for (int lane = 0; lane < POLICY_WAVE; ++lane) reads(off + wide_last_word(g, lane), 4);
  return end;
}

// ------------------------------------------------------------------ device side
#ifdef __HIPCC__
typedef float pw_v16 __attribute__((ext_vector_type(16)));
typedef float pw_v4 __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1))) pw_gfloat;
typedef const pw_v4 __attribute__((address_space(1))) pw_gv4;

// a's lanes 32 .. 63 <-> b's lanes 0 .. 31
__device__ __forceinline__ void wide_swap(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}

__device__ __forceinline__ pw_v4 wide_load4(pw_gfloat* p) { return *reinterpret_cast<pw_gv4*>(p); }

// the accumulators of a tile, started from its bias: the 16 words of this lane's half
__device__ __forceinline__ pw_v16 wide_bias(pw_gfloat* tile, int lane) {
  pw_gfloat* const p = tile + wide_bias_word(lane >> 5);
  const pw_v4 b0 = wide_load4(p), b1 = wide_load4(p + 4), b2 = wide_load4(p + 8), b3 = wide_load4(p + 12);
  pw_v16 acc;
#pragma unroll
  for (int i = 0; i < 4; ++i) { acc[i] = b0[i]; acc[4 + i] = b1[i]; acc[8 + i] = b2[i]; acc[12 + i] = b3[i]; }
  return acc;
}

// four k-steps: the A operands of group g of the area at `a` (one 16-byte load per lane), the B operands b[0 .. 3]
__device__ __forceinline__ void wide_group(pw_gfloat* a, int word, const float* b, pw_v16& acc) {
  const pw_v4 w = wide_load4(a + word);
#pragma unroll
  for (int k = 0; k < 4; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[k], b[k], acc, 0, 0, 0);
}

// relu of a result tile and its 16 registers as the next layer's 16 k-steps (wide_reorder_kstep)
__device__ __forceinline__ void wide_relu_reorder(const pw_v16& acc, float (&b)[16]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float r0 = fmaxf(acc[4 * q], 0.f), r1 = fmaxf(acc[4 * q + 1], 0.f), r2 = fmaxf(acc[4 * q + 2], 0.f), r3 = fmaxf(acc[4 * q + 3], 0.f);
    wide_swap(r0, r1);
    wide_swap(r2, r3);
    b[4 * q] = r0; b[4 * q + 2] = r1; b[4 * q + 1] = r2; b[4 * q + 3] = r3;
  }
}

// the last layer's share of one tile of its input: 16 k-steps from group 4 t on
__device__ __forceinline__ void wide_last_tile(pw_gfloat* wl, int t, int lane, const float (&b)[16], pw_v16& last) {
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) wide_group(wl, wide_last_word(4 * t + gg, lane), &b[4 * gg], last);
}

// The actions of the wavefront's 64 envs, each lane its own env's, from the observation rows x (one env per lane).
// `blk`, `pol_off`, z, act, logp: as policy_eval_impl (salp_policy.h).
template <int AD, bool SAMPLED>
__device__ __forceinline__ void policy_eval_wide(const float* blk, uint32_t pol_off, const float (&x)[WIDE_OBS], [[maybe_unused]] const float (&z)[AD],
                                                 float (&act)[AD], [[maybe_unused]] float& logp) {
  static_assert(AD >= 1 && 2 * AD <= WIDE_ROWS, "mean and log-std rows share the last layer's four rows");
  pol_int* hd = policy_block_header(blk);
  asm volatile("" : "+s"(hd));
  const int nh = hd[PH_NHIDDEN], h0 = hd[PH_H0], h1 = hd[PH_H1], out_act = hd[PH_OUT];
  const uint32_t base = PH_WORDS + (uint32_t)__builtin_amdgcn_readfirstlane((int)pol_off);
  pw_gfloat* const w = (pw_gfloat*)(uintptr_t)hd + base;
  const int lane = (int)(threadIdx.x & (POLICY_WAVE - 1));
  const int t0n = h0 / WIDE_TILE, t1n = h1 / WIDE_TILE;
  const int tile1_words = wide_tile_words(h0);
  const int l0_words = t0n * wide_tile_words(WIDE_OBS);
  const int tail_off = l0_words + (nh >= 2 ? t1n * tile1_words : 0);
  const pol_v8 tl = pol_load8((pol_float*)hd + base + tail_off);     // the last rows' biases, scale, shift
  pw_gfloat* const wl = w + tail_off + POLICY_TAIL_WORDS;

  // the observations as B operands: k-step s of envs 0 .. 31 and of envs 32 .. 63
  float xb0[WIDE_OBS / 2], xb1[WIDE_OBS / 2];
#pragma unroll
  for (int s = 0; s < WIDE_OBS / 2; ++s) {
    float a = x[2 * s], b = x[2 * s + 1];
    wide_swap(a, b);
    xb0[s] = a; xb1[s] = b;
  }
  float res0[WIDE_ROWS], res1[WIDE_ROWS];
#pragma unroll
  for (int r = 0; r < WIDE_ROWS; ++r) res0[r] = res1[r] = 0.f;

#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    float xb[WIDE_OBS / 2];
#pragma unroll
    for (int s = 0; s < WIDE_OBS / 2; ++s) xb[s] = half ? xb1[s] : xb0[s];
    pw_v16 last;
#pragma unroll
    for (int r = 0; r < 16; ++r) last[r] = r < WIDE_ROWS ? tl[r] : 0.f;
    if (nh == 1) {
#pragma unroll 1
      for (int t = 0; t < t0n; ++t) {
        pw_gfloat* const wt = w + t * wide_tile_words(WIDE_OBS);
        pw_v16 acc = wide_bias(wt, lane);
#pragma unroll
        for (int g = 0; g < WIDE_OBS / 8; ++g) wide_group(wt + WIDE_TILE, wide_a_word(g, lane), &xb[4 * g], acc);
        float tb[16];
        wide_relu_reorder(acc, tb);
        wide_last_tile(wl, t, lane, tb, last);
      }
    } else {
      float hb[WIDE_MAX_HIDDEN / WIDE_TILE][16];     // the first hidden layer of this half, as B operands
#pragma unroll
      for (int t = 0; t < WIDE_MAX_HIDDEN / WIDE_TILE; ++t) {
        if (t < t0n) {
          pw_gfloat* const wt = w + t * wide_tile_words(WIDE_OBS);
          pw_v16 acc = wide_bias(wt, lane);
#pragma unroll
          for (int g = 0; g < WIDE_OBS / 8; ++g) wide_group(wt + WIDE_TILE, wide_a_word(g, lane), &xb[4 * g], acc);
          wide_relu_reorder(acc, hb[t]);
        } else {
#pragma unroll
          for (int j = 0; j < 16; ++j) hb[t][j] = 0.f;
        }
      }
      pw_gfloat* const w1 = w + l0_words;
#pragma unroll 1
      for (int t = 0; t < t1n; ++t) {
        pw_gfloat* const wt = w1 + t * tile1_words;
        pw_v16 acc = wide_bias(wt, lane);
#pragma unroll
        for (int g8 = 0; g8 < WIDE_MAX_HIDDEN / WIDE_TILE; ++g8) {
          if (g8 < t0n) {
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) wide_group(wt + WIDE_TILE, wide_a_word(4 * g8 + gg, lane), &hb[g8][4 * gg], acc);
          }
        }
        float tb[16];
        wide_relu_reorder(acc, tb);
        wide_last_tile(wl, t, lane, tb, last);
      }
    }
    // rows 0 .. 3 of the last layer sit in registers 0 .. 3 of lanes 0 .. 31 (wide_cd_row), one env per lane
    if (half == 0) {
#pragma unroll
      for (int r = 0; r < WIDE_ROWS; ++r) res0[r] = last[r];
    } else {
#pragma unroll
      for (int r = 0; r < WIDE_ROWS; ++r) res1[r] = last[r];
    }
  }
  // back to one env per lane: the second half's results move to lanes 32 .. 63
#pragma unroll
  for (int r = 0; r < (SAMPLED ? 2 * AD : AD); ++r) wide_swap(res0[r], res1[r]);

  // ---- the tail: policy_eval_impl's operations, in its order
  if constexpr (SAMPLED) {
    float lp = 0.f;
#pragma unroll
    for (int a = 0; a < AD; ++a) {
      const float l = fminf(fmaxf(res0[AD + a], -20.0f), 2.0f);
      const float sd = expf(l);
      const float s = __builtin_fmaf(sd, z[a], res0[a]);
      const float m2 = -2.0f * s;
      const float sp = fmaxf(m2, 0.f) + log1pf(expf(-fabsf(m2)));
      const float c = (0.693147180559945309f - s) - sp;
      float g = -0.5f * (z[a] * z[a]);
      g = g - l;
      g = g - 0.918938533204672742f;
      g = g - 2.0f * c;
      lp = lp + g;
      act[a] = tanhf(s) * tl[WIDE_TAIL_SCALE + a] + tl[WIDE_TAIL_SHIFT + a];
    }
    logp = lp;
  } else {
#pragma unroll
    for (int a = 0; a < AD; ++a) {
      const float v = out_act ? fminf(fmaxf(res0[a], -1.0f), 1.0f) : tanhf(res0[a]);
      act[a] = v * tl[WIDE_TAIL_SCALE + a] + tl[WIDE_TAIL_SHIFT + a];
    }
  }
}
#endif  // __HIPCC__

}  // namespace salp
