// wide_policy_host.cpp — host twin of the wide in-kernel policy (TEST INFRASTRUCTURE).
// Compiles the host section of csrc/salp_policy_wide.h as plain C++ (oracle/Makefile's pattern rule for tests/*_host.cpp) and
// exports, next to it:
//   salp_wide_policy_forward / _gaussian   an fmaf restatement of the arithmetic include/salp_vec.h promises, for widths up
//                                          to 256, written from the PUBLIC weight layout alone (no block, no map);
//   salp_wide_policy_emulate               the kernel's data flow replayed on 64 host "lanes" from a device block: the lane
//                                          swaps, the 32 x 32 x 2 products under the operand maps the header documents,
//                                          the eight-swap reorder — every address formed by the header's own constexpr maps.
#include <math.h>
#include <string.h>

#include "../underwater-swimmer_rl_amd/csrc/salp_policy_wide.h"

using namespace salp;

namespace {

// y = W x + b: bias first, one fmaf per input in ascending index order; relu = fmaxf(., 0)
void layer(const float* W, const float* b, int in, int out, const float* x, float* y, bool relu) {
  for (int j = 0; j < out; ++j) {
    float s = b[j];
    for (int i = 0; i < in; ++i) s = fmaf(W[(size_t)j * in + i], x[i], s);
    y[j] = relu ? fmaxf(s, 0.f) : s;
  }
}

// the hidden layers of one policy in the public layout; returns the last width and leaves its activations in x
int body(const salp_policy_desc_t* d, const float*& p, float* x) {
  int in = WIDE_OBS;
  float y[WIDE_MAX_HIDDEN];
  for (int l = 0; l < d->n_hidden; ++l) {
    const int out = d->hidden[l];
    layer(p, p + (size_t)out * in, in, out, x, y, true);
    memcpy(x, y, sizeof(float) * out);
    p += (size_t)out * in + out;
    in = out;
  }
  return in;
}

bool shape_ok(const salp_policy_desc_t* d, int act_dim) {
  if (!d || d->n_hidden < 1 || d->n_hidden > 2 || act_dim < 1 || act_dim > 2) return false;
  for (int l = 0; l < d->n_hidden; ++l)
    if (d->hidden[l] < 1 || d->hidden[l] > WIDE_MAX_HIDDEN) return false;
  return true;
}

// ---- the emulation: a register is 64 lane values
struct Reg { float v[POLICY_WAVE]; };
void swap32(Reg& a, Reg& b) {     // a's lanes 32 .. 63 <-> b's lanes 0 .. 31
  for (int l = 0; l < 32; ++l) { const float t = a.v[32 + l]; a.v[32 + l] = b.v[l]; b.v[l] = t; }
}
struct Acc { Reg r[16]; };
// D = A B + C with A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31], C/D by wide_cd_row: k = 0, then k = 1
void mfma(const Reg& a, const Reg& b, Acc& c) {
  for (int lane = 0; lane < POLICY_WAVE; ++lane)
    for (int reg = 0; reg < 16; ++reg) {
      const int i = wide_cd_row(reg, lane), j = lane & 31;
      float s = c.r[reg].v[lane];
      for (int k = 0; k < 2; ++k) s = fmaf(a.v[32 * k + i], b.v[32 * k + j], s);
      c.r[reg].v[lane] = s;
    }
}
void bias(const float* tile, Acc& acc) {
  for (int lane = 0; lane < POLICY_WAVE; ++lane)
    for (int reg = 0; reg < 16; ++reg) acc.r[reg].v[lane] = tile[wide_bias_word(lane >> 5) + reg];
}
void group(const float* area, bool last, int g, const Reg* b, Acc& acc) {
  for (int k = 0; k < 4; ++k) {
    Reg a;
    for (int lane = 0; lane < POLICY_WAVE; ++lane) a.v[lane] = area[(last ? wide_last_word(g, lane) : wide_a_word(g, lane)) + k];
    mfma(a, b[k], acc);
  }
}
void relu_reorder(const Acc& acc, Reg* b) {
  for (int q = 0; q < 4; ++q) {
    Reg r[4];
    for (int i = 0; i < 4; ++i)
      for (int lane = 0; lane < POLICY_WAVE; ++lane) r[i].v[lane] = fmaxf(acc.r[4 * q + i].v[lane], 0.f);
    swap32(r[0], r[1]);
    swap32(r[2], r[3]);
    b[4 * q] = r[0]; b[4 * q + 2] = r[1]; b[4 * q + 1] = r[2]; b[4 * q + 3] = r[3];
  }
}

}  // namespace

extern "C" {

int salp_wide_policy_host_check(int obs_dim, int act_dim, int kmax, int food_slots, int64_t n_envs, const salp_policy_desc_t* d,
                                int gaussian, int* words, const char** why) {
  const char* msg = "";
  const int rc = check_policy_desc_wide(obs_dim, act_dim, kmax, food_slots, n_envs, d, gaussian != 0, words, &msg);
  if (why) *why = msg;
  return rc;
}

// policy_block_map_wide(): the stride; the first min(stride, capacity) entries go to map (nullable)
int salp_wide_policy_host_map(int act_dim, const salp_policy_desc_t* d, int gaussian, int32_t* map, int capacity) {
  std::vector<int32_t> m;
  const int stride = policy_block_map_wide(act_dim, *d, gaussian != 0, m);
  for (int k = 0; map && k < stride && k < capacity; ++k) map[k] = m[k];
  return stride;
}

void salp_wide_policy_host_header(const salp_policy_desc_t* d, int stride, int64_t n_envs, int gaussian, int32_t* hd) {
  int32_t w[PH_WORDS];
  policy_header_wide(*d, stride, n_envs, gaussian != 0, w);
  for (int i = 0; i < PH_WORDS; ++i) hd[i] = w[i];
}

int salp_wide_policy_host_read_end(const salp_policy_desc_t* d) { return policy_wide_read_end(*d); }

// the shared constexpr maps, by code: 0 cd_row(a, b)  1 a_word(a, b)  2 last_word(a, b)  3 bias_word(a)  4 tile_words(a)
// 5 reorder_kstep(a)  6 PH_WIDE  7 ab_index(a)  8 ab_k(a)
int salp_wide_policy_host_index(int code, int a, int b) {
  switch (code) {
    case 0: return wide_cd_row(a, b);
    case 1: return wide_a_word(a, b);
    case 2: return wide_last_word(a, b);
    case 3: return wide_bias_word(a);
    case 4: return wide_tile_words(a);
    case 5: return wide_reorder_kstep(a);
    case 6: return PH_WIDE;
    case 7: return wide_ab_index(a);
    case 8: return wide_ab_k(a);
    default: return -1;
  }
}

// u [M][act_dim] (before the output activation, nullable) and a [M][act_dim] of ONE policy in the public layout
int salp_wide_policy_forward(const salp_policy_desc_t* desc, int32_t act_dim, const float* weights, const float* obs, int64_t M,
                             float* u, float* a) {
  if (!shape_ok(desc, act_dim) || !weights || !obs || !a || M < 0) return -1;
  for (int64_t m = 0; m < M; ++m) {
    float x[WIDE_MAX_HIDDEN], y[2];
    memcpy(x, obs + m * WIDE_OBS, sizeof(float) * WIDE_OBS);
    const float* p = weights;
    const int in = body(desc, p, x);
    layer(p, p + (size_t)act_dim * in, in, act_dim, x, y, false);
    const float* scale = p + (size_t)act_dim * in + act_dim;
    const float* shift = scale + act_dim;
    for (int k = 0; k < act_dim; ++k) {
      const float t = desc->out_activation == SALP_POLICY_OUT_CLIP ? fminf(fmaxf(y[k], -1.0f), 1.0f) : tanhf(y[k]);
      const float prod = t * scale[k];
      if (u) u[m * act_dim + k] = y[k];
      a[m * act_dim + k] = prod + shift[k];
    }
  }
  return 0;
}

// the mean head m and the log-std head's raw sum r, [M][act_dim] each, of ONE policy in the public Gaussian layout
int salp_wide_policy_forward_gaussian(const salp_policy_desc_t* desc, int32_t act_dim, const float* weights, const float* obs,
                                      int64_t M, float* m_out, float* r_out) {
  if (!shape_ok(desc, act_dim) || !weights || !obs || !m_out || !r_out || M < 0) return -1;
  for (int64_t m = 0; m < M; ++m) {
    float x[WIDE_MAX_HIDDEN];
    memcpy(x, obs + m * WIDE_OBS, sizeof(float) * WIDE_OBS);
    const float* p = weights;
    const int in = body(desc, p, x);
    const float* W_mu = p;
    const float* b_mu = W_mu + (size_t)act_dim * in;
    const float* W_ls = b_mu + act_dim;
    const float* b_ls = W_ls + (size_t)act_dim * in;
    layer(W_mu, b_mu, in, act_dim, x, m_out + m * act_dim, false);
    layer(W_ls, b_ls, in, act_dim, x, r_out + m * act_dim, false);
  }
  return 0;
}

// The sums of the last layer's four rows for one wavefront, rows [64][4], from ONE policy's words of a device block
// (`block`: its `stride` words, as the map lays them out) and 64 observation rows.  Every index at or beyond `stride`
// that the replay would read is counted in the return value instead of being read (0: none).
int salp_wide_policy_emulate(const salp_policy_desc_t* d, const float* block, int stride, const float* obs, float* rows) {
  int beyond = 0;
  std::vector<float> w((size_t)stride + 4096 * 16, 0.f);     // reads past the stride land in zeros and are counted below
  memcpy(w.data(), block, sizeof(float) * stride);
  if (policy_wide_read_end(*d) > stride) beyond = policy_wide_read_end(*d) - stride;
  const int nh = d->n_hidden, h0 = d->hidden[0], h1 = d->hidden[1];
  const int t0n = h0 / WIDE_TILE, t1n = h1 / WIDE_TILE;
  const int l0_words = t0n * wide_tile_words(WIDE_OBS), tile1_words = wide_tile_words(h0);
  const int tail_off = l0_words + (nh >= 2 ? t1n * tile1_words : 0);
  const float* tl = w.data() + tail_off;
  const float* wl = tl + POLICY_TAIL_WORDS;
  Reg x[WIDE_OBS], xb[2][WIDE_OBS / 2];
  for (int i = 0; i < WIDE_OBS; ++i)
    for (int lane = 0; lane < POLICY_WAVE; ++lane) x[i].v[lane] = obs[lane * WIDE_OBS + i];
  for (int s = 0; s < WIDE_OBS / 2; ++s) {
    Reg a = x[2 * s], b = x[2 * s + 1];
    swap32(a, b);
    xb[0][s] = a; xb[1][s] = b;
  }
  Reg res[2][WIDE_ROWS];
  for (int half = 0; half < 2; ++half) {
    Acc last;
    for (int reg = 0; reg < 16; ++reg)
      for (int lane = 0; lane < POLICY_WAVE; ++lane) last.r[reg].v[lane] = reg < WIDE_ROWS ? tl[reg] : 0.f;
    std::vector<Reg> hb((size_t)16 * (WIDE_MAX_HIDDEN / WIDE_TILE));
    for (int t = 0; t < t0n; ++t) {
      const float* wt = w.data() + t * wide_tile_words(WIDE_OBS);
      Acc acc;
      bias(wt, acc);
      for (int g = 0; g < WIDE_OBS / 8; ++g) group(wt + WIDE_TILE, false, g, &xb[half][4 * g], acc);
      relu_reorder(acc, &hb[16 * t]);
      if (nh == 1)
        for (int gg = 0; gg < 4; ++gg) group(wl, true, 4 * t + gg, &hb[16 * t + 4 * gg], last);
    }
    for (int t = 0; nh == 2 && t < t1n; ++t) {
      const float* wt = w.data() + l0_words + t * tile1_words;
      Acc acc;
      bias(wt, acc);
      for (int g = 0; g < 4 * t0n; ++g) group(wt + WIDE_TILE, false, g, &hb[4 * g], acc);
      Reg tb[16];
      relu_reorder(acc, tb);
      for (int gg = 0; gg < 4; ++gg) group(wl, true, 4 * t + gg, &tb[4 * gg], last);
    }
    for (int r = 0; r < WIDE_ROWS; ++r) res[half][r] = last.r[r];
  }
  for (int r = 0; r < WIDE_ROWS; ++r) {
    swap32(res[0][r], res[1][r]);
    for (int lane = 0; lane < POLICY_WAVE; ++lane) rows[lane * WIDE_ROWS + r] = res[0][r].v[lane];
  }
  return beyond;
}

}  // extern "C"
