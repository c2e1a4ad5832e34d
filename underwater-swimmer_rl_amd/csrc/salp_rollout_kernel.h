// salp_rollout_kernel.h — the fused SALP step/rollout kernel for gfx950 and the choice among its instantiations.
//
// Kernel design:
//   * one SALP per lane, 256-thread workgroups (4 wavefronts), env index = blockIdx*256 + tid;
//   * state is struct-of-arrays in HBM (row-major [quantity][env], 8-byte and 4-byte rows), read
//     once at kernel entry, held in VGPRs across the `horizon` steps, written once at exit;
//   * per step each wavefront stages its 64 observation rows (64 x obs_dim floats) in its private
//     LDS tile and streams them out as whole 16-byte-per-lane coalesced stores, so the
//     [horizon][n_envs][obs_dim] row-major output is written as contiguous 64*obs_dim*4-byte
//     runs per wavefront; actions are prefetched one step ahead;
//   * episode / reward statistics are reduced with wavefront shuffles, then one 64-bit integer
//     atomic per block and statistic into one of 64 line-sized replicas (order-independent).
// No MFMA: there is no dense contraction on this path; the bound is HBM write bandwidth.
//
// The template is instantiated implicitly, by the small salp_rollout_*.hip units next to this file: one per food-slot count
// and literal / run-time constants for K = 3, one for the generic-K kernels, so that the 360 instantiations compile in
// parallel.  Each unit defines the rollout_unit_fn of its handle class (the generic unit: of its two); salp_vec.hip (the
// service kernels and the C ABI of include/salp_vec.h) reaches the kernels only through those.  No instantiation may be
// named in two units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>

#include <type_traits>

#include "../../include/salp_vec.h"
#include "salp_device.h"
#include "salp_food_lds.h"
#include "salp_food_reg.h"
#include "salp_policy.h"

using namespace salp;

// What a choice of kernel returns: the kernel (its host-side address, a rollout_fn) and the output signature it was
// compiled for — which is not always the one asked for (pick_sig): salp_vec_last_launch / _signatures report this value.
struct RolloutPick {
  const void* fn;
  int sig;
#ifdef SALP_EXP_STAMPS   // experiment builds only: readers of the choosing unit's own copy of the __device__ globals
  int (*read_stamps)(uint32_t* dst, int words);
#endif
#ifdef SALP_EXP_COUNT
  int (*read_counters)(unsigned long long* dst);
#endif
};
// One per handle class (a handle uses the same one for its whole life): the kernel for a launch's form (predicated or
// not), breathing mode, wanted output signature (kSig*) and action source (ACT_*).
typedef RolloutPick (*rollout_unit_fn)(bool ragged, bool forced, int sig, int act);
#define SALP_ROLLOUT_UNIT(name) __attribute__((visibility("hidden"))) RolloutPick name(bool ragged, bool forced, int sig, int act)
SALP_ROLLOUT_UNIT(salp_rollout_f1_std);   SALP_ROLLOUT_UNIT(salp_rollout_f1_rt);    // K = 3: food slots x literal (std) /
SALP_ROLLOUT_UNIT(salp_rollout_f4_std);   SALP_ROLLOUT_UNIT(salp_rollout_f4_rt);    // run-time (rt) constants, one unit each
SALP_ROLLOUT_UNIT(salp_rollout_f8_std);   SALP_ROLLOUT_UNIT(salp_rollout_f8_rt);
SALP_ROLLOUT_UNIT(salp_rollout_f12_std);  SALP_ROLLOUT_UNIT(salp_rollout_f12_rt);
SALP_ROLLOUT_UNIT(salp_rollout_f16_std);  SALP_ROLLOUT_UNIT(salp_rollout_f16_rt);
SALP_ROLLOUT_UNIT(salp_rollout_generic12); SALP_ROLLOUT_UNIT(salp_rollout_generic16);  // K != 3: salp_rollout_generic.hip

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int kBlock = 256;
constexpr int kWave = 64;
// Wavefronts per SIMD the launch bounds ask for (workgroups of 256 threads per CU), by food-slot count:
//   one food 4;  4 / 8 slots 4 — 128 VGPRs, their LDS (32 / 40 KB) allows four workgroups per CU; without the bound several
//   signatures landed on 129 = three per SIMD, up to 22 % slower (profiles/r03/ab_notes.md sessions 14, 20);  12 slots 3 —
//   <= 168 VGPRs, 49 KB of LDS (four: a timing build at 128 VGPRs / 36 KB was 13 % slower, session 17);  16 slots 3 for the
//   literal-constant unpredicated kernels (half-height tile, session 19), else 2;  generic K: 2 (12 slots) / 1 (16 slots).
//   The packed signature keeps every row (its 8-slot kernel keeps the six-column tile, TAILREG below); its one-wavefront
//   predicated 8-slot twin has the seven-column tile, 45 KB: 3.
//   The policy kernels (ACT_POLICY): the first hidden layer's activations are up to 64 VGPRs on top of the step's own.  One food
//   and 4 slots: 2 (256 registers, no scratch).  8 slots and more, and every predicated launch: 1 — at 2 they spilled 50-580 B
//   per lane to scratch inside the step loop; at 1 the wavefront owns the SIMD's 512 registers and what does not fit in the
//   256 VGPRs is parked in AGPRs (v_accvgpr_write / _read), not in memory (profiles/r05/policy_kernel_resources.txt).
constexpr int waves_per_simd(int fmax, int kmax, bool std_consts, bool ragged, int sig, bool policy = false, bool sampled = false,
                             bool forced = false) {
  // The sampling policy kernels (ACT_POLICY_SAMPLED) take their deterministic twins' bounds, but for six unpredicated kernels
  // that at 2 held 2-16 scratch instructions (12-36 B per lane) where the twin holds fewer or none — the 4-slot rollout kernels,
  // the free-breathing 4-slot summary kernel with literal constants, the free-breathing one-food summary kernel with run-time
  // constants: 1.  From the code-object metadata of all 80: profiles/r07/sampled_kernel_resources.txt.
  if (sampled && !ragged && fmax == 4 && (sig == 1 || !forced)) return 1;
  if (sampled && !ragged && fmax == 1 && sig == 4 && !std_consts && !forced) return 1;
  // The summary kernels (sig 4) take their twins' bounds, but for the unpredicated 4-slot kernel with run-time constants: 1 (at 2
  // it sat at 255-256 VGPRs with 12-132 B of scratch, its twin holds 0-12 B; at 1 258-272 registers, 2-16 of them AGPRs, none).
  // From the code-object metadata of all 40: profiles/r06/eval_kernel_resources.txt.
  if (policy && sig == 4 && fmax == 4 && !std_consts && !ragged) return 1;
  // The navigation kernels (sig 5, one food): 1 — the record and the trial's line are 26 more registers across the loop than the
  // summary kernel's 224; at 2 the unpredicated kernel with literal constants held 136 B of scratch (33 VGPRs spilled).
  if (policy && sig == 5) return 1;
  if (policy) return (ragged || fmax >= 8) ? 1 : 2;
  if (sig == 3 && ragged && kmax == 3 && fmax == 8) return 3;
  return fmax <= 1 ? 4 : (kmax != 3 ? (fmax <= 12 ? 2 : 1) : (fmax <= 8 ? 4 : (fmax <= 12 ? 3 : ((std_consts && !ragged) ? 3 : 2))));
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

struct IOPtrs {
  const float* act;       // [H][n][act_dim] or null (device-generated); ACT_POLICY: the policy's device block (salp_policy.h)
  float* obs;             // [H][n][obs_dim]
  union {
    float* reward;        // [H][n]
    const double* nav_line;   // kSigNav: [n][4] start x, start y, goal x, goal y
  };
  uint8_t* terminated;    // [H][n]
  uint8_t* truncated;     // [H][n]
  float* final_obs;       // [H][n][obs_dim] rows of finished envs only
  union {
    int32_t* info;        // [H][n][3]
    float* logp_out;      // ACT_POLICY_SAMPLED (whose signatures have no info): [H][n] or null
  };
  union {
    float* act_out;       // [H][n][act_dim]
    double* nav_track;    // kSigNav: [H][n][2] position after each step of the call, or null
  };
  DevStats* stats;        // [SALP_STATS_REPLICAS] or null
  union {
    int64_t global_step;  // step index of t = 0 (device-generated actions)
    double nav_radius;    // kSigNav (no generated actions): the goal radius
  };
};

#ifdef SALP_EXP_STAMPS
constexpr int kStampWaves = 8192;
__device__ uint32_t salp_stamp_out[kStampWaves * 16];
#endif

// Device-memory copy of the launch constants for the RARE paths of the rollout kernel (respawn / autoreset
// region, exact capture pass, state write-back).  Everything the per-step path needs arrives by value in
// `P` (scalar registers); what only the rare paths read is fetched from this block when they run, so it
// does not occupy scalar registers across the step loop (the by-value copy alone left ~125 SGPRs spilled
// to VGPR lanes, ~110 v_readlane / v_writelane per step in the 12-food kernel).  Immutable after create;
// base_num_food_items, the one field a caller may change between launches, is always taken from `P`.
struct ColdBlock {
  DevParams P;
  DevState S;
  uint32_t seed[2];   // the key of the draw streams: P.seed (in every copy of P) points here
};

// FULL = the common rollout signature (act, obs, reward, terminated, truncated all present; no
// final_obs / info): no per-step null tests.
// RAGGED = false: every wavefront of the launch is either full (64 envs) or empty, so no store is
// predicated and the compiler can count the stores issued after the action prefetch (it then waits
// for the prefetch alone instead of draining all stores with s_waitcnt vmcnt(0) every step).
// RAGGED = true: the same loop with per-lane predicates; the host launches it for the last
// n % 64 envs only (one wavefront).  `env_begin/env_end`: the env range of this launch.
// GEN = actions are generated in the kernel (salp_vec_rollout with act == NULL): no read stream at
// all — the per-step 256-B action read costs the write stream ~10 % (HBM read/write turnarounds,
// profiles/r01/ab_notes.md) — and, if act_out is given, the actions are written out instead.
// ACT = ACT_POLICY: the actions are a function of the observations (salp_vec_rollout_policy): the action of step 0 is the
// policy (salp_policy.h) applied to the env's current observation, computed in the prologue with the step's own
// functions; the action of step t + 1 is the policy applied to the row just written to obs[t], evaluated from the
// registers behind the tile flush, while the row stores drain.  No read stream; act_out as with ACT_GEN.
// ACT = ACT_POLICY_SAMPLED: the same closed loop with the stochastic form of a Gaussian policy (salp_vec_rollout_policy_sampled,
// salp_vec_evaluate_policy_sampled): the action of step t is sampled with the policy's noise block n0 + t of the env, n0 =
// the policy's noise step read from its device block at entry; its log-probability goes to logp_out with the action.
enum { ACT_READ = 0, ACT_GEN = 1, ACT_POLICY = 2, ACT_POLICY_SAMPLED = 3 };
template <int FMAX, int KMAX, bool FORCED, bool STD, int SIG, bool RAGGED, int ACT>
__global__ __launch_bounds__(kBlock, waves_per_simd(FMAX, KMAX, STD, RAGGED, SIG, ACT >= ACT_POLICY, ACT == ACT_POLICY_SAMPLED, FORCED)) void salp_rollout_kernel(DevParams P_arg, DevState S, IOPtrs io, int H, int64_t env_begin, int64_t env_end, const ColdBlock* __restrict__ cold) {
  // STD = false: where the hot path's constants come from (open_consts, salp_device.h) — the device copy, function by
  // function, for the 4- and 8-slot kernels; the by-value launch parameters for the others
  constexpr bool GEN = ACT == ACT_GEN;
  constexpr bool SAMPLED = ACT == ACT_POLICY_SAMPLED;
  constexpr bool POLICY = ACT == ACT_POLICY || SAMPLED;
  // SIG 4 (kSigSummary): NO per-step output at all — salp_vec_evaluate_policy.  io.obs is the block of per-env summary records
  // ([n][SALP_EVAL_WORDS] words, include/salp_vec.h), io.final_obs non-NULL says that the records are read first and continued
  // (SALP_EVAL_ACCUMULATE).  The observation is formed in registers for the policy alone: no tile write, no flush, no
  // reward / flag / action store; the record leaves next to the state write-back.  The LDS layout is that of the twin policy
  // kernel (the rare paths still borrow the tile's bytes, the mirror sits behind it): LDS limits none of these kernels.
  // SIG 5 (kSigNav): the summary kernel's loop with a per-env `running` predicate and a navigation record — salp_vec_evaluate_navigation.
  // io.obs is the block of records ([n][SALP_NAV_WORDS] words), io.final_obs non-NULL = SALP_EVAL_ACCUMULATE, io.nav_line the
  // trials' start / goal, io.nav_radius the goal radius, io.nav_track the optional positions.  A lane that is not running is not
  // stepped: nothing of its state, statistics or record moves; a wavefront with no running lane leaves the step loop.
  constexpr bool NAV = SIG == 5;
  constexpr bool SUMMARY = SIG == 4 || NAV;     // everything the two share: no per-step output, no tile write
  static_assert(!POLICY || ((SIG == 1 || SIG == 4 || SIG == 5) && KMAX == 3), "policy kernels: the main-only, the summary and the navigation signature, K = 3");
  static_assert(!SUMMARY || POLICY, "the summary signature exists for the in-kernel policy only");
  static_assert(!NAV || (FMAX == 1 && FORCED && ACT == ACT_POLICY), "the navigation signature: one food, forced breathing, the deterministic policy");
  // (the summary kernels the other way round — by value with 4 / 8 slots, the device copy with 16: with no store in the step loop
  // the twins' choice left 300-560 scalar registers spilled and 68-196 B of scratch reserved in four of them; so chosen, none
  // of the 40 holds scratch where its twin holds none, profiles/r06/eval_kernel_resources.txt)
  constexpr bool MEMC = !STD && KMAX == 3 && (SIG == 4 ? FMAX == 16 : (FMAX == 4 || FMAX == 8));
  DevParams P_pol = P_arg;
  P_pol.use_mem = MEMC ? 1 : 0;
  const DevParams& P = STD ? P_arg : P_pol;
  constexpr bool FULL = SIG != 0;         // obs, reward, terminated, truncated all present: their stores are unconditional
  constexpr bool EXTRAS = SIG != 1 && !SUMMARY;   // final_obs / info may be present (tested per use; SIG 0: every output is tested)
  // SIG 3 (kSigPacked): ONE output stream of transition records (include/salp_vec.h "Packed transition record") — the
  // observation row plus one float4 (reward, flags word, food_collected, steps_since_food) — through the tile; io.obs is
  // the record block, io.final_obs non-NULL says that the rows carry a terminal-observation tail
  constexpr bool PACKED = SIG == 3;
  // TAILREG: the unpredicated 8-slot packed kernel stores that last float4 straight from registers (one 16-B store per
  // lane where the other signatures issue their reward / flag / info stores) and keeps the tile of the unpacked
  // signatures: 40960 B of LDS per workgroup is exactly four workgroups per CU, a seven-column tile (45056 B) is three.
  constexpr bool TAILREG = PACKED && !RAGGED && KMAX == 3 && FMAX == 8;
  constexpr int QMAX = 3 + KMAX;          // float4 per observation row
  constexpr int QPMAX = QMAX + ((PACKED && !TAILREG) ? 1 : 0);   // float4 columns of a tile row
  // LDS tile of the wavefront's 64 observation rows.  Banking (MI355X_MICROARCH.md §LDS): ds_write_b128 goes
  // in 8 groups of 8 lanes over banks (a/4) mod 32, ds_read_b128 in 4 groups of 16 lanes ({0-3,12-15,20-27},
  // ...) over banks (a/4) mod 64.  K = 3 (Q = 6 float4 per row): unpadded 96-B rows with the float4 column
  // XOR-ed by bit 2 of the row — conflict-free for the row writes AND for the flush reads (profiles/isa_lds_model.py;
  // the 112-B padded pitch of round 1 was conflict-free for the writes only: 2-way on the reads).
  // Other K (generic instantiation, Q possibly odd): the padded pitch.
  // PACKED: unpadded rows of Q + 1 float4 with no swizzle.  K = 3: 7 float4 = 112 B, an ODD number of float4, so eight
  // consecutive rows start in eight different 16-B bank groups (writes conflict-free) and the flush reads float4 j*64 + lane
  // of a linear tile (reads conflict-free): profiles/isa_lds_model.py PACKED.  Generic K: rows of QPMAX float4, not modelled.
  constexpr bool SWZ = (KMAX == 3) && (!PACKED || TAILREG);
  constexpr int PITCH = (PACKED && !TAILREG) ? 4 * QPMAX : (SWZ ? 4 * QMAX : 4 * QMAX + 4);     // LDS row pitch in floats
  // Where the food positions of a multi-food env live: up to 12 slots in VGPRs with an fp32 mirror in LDS
  // (salp_food_reg.h), above that in LDS (salp_food_lds.h); one food is plain registers.
  constexpr bool REGF = FMAX > 1 && (FMAX <= 12 || KMAX == 3);   // K = 3: every slot count; generic K: up to 12 slots
  constexpr bool LDSF = FMAX > 1 && !REGF;                         // generic K with 13..16 slots
  constexpr bool MULTI = REGF || LDSF;
  double2* food_lds = nullptr;
  if constexpr (LDSF) {     // (declared only where it exists: a one-element stand-in would cost the 8-slot kernel its fourth workgroup per CU)
    __shared__ __attribute__((aligned(16))) double2 food_lds_block[(kBlock / kWave) * FMAX * kWave];
    food_lds = food_lds_block;
  }
  // Per-wavefront LDS region: the observation tile (64 rows of PITCH floats) and, for the register-food kernels, the
  // fp32 mirror of the food positions behind it (8 B per slot and lane, salp_food_reg.h; lives for the whole launch).
  // 12 slots, K = 3: 6144 + 6144 B per wavefront, 49 KB per workgroup -> 3 workgroups per CU.  The tile's bytes, idle in
  // the middle of a step, are lent to the rare paths as scratch: the exact order's distances (8 B per slot and lane,
  // <= the tile for every instantiation) and the placement's accepted points.
  // HALF: a tile of 32 rows, written and flushed twice per step (lanes 0-31, then 32-63): 3072 instead of 6144 B per wavefront.
  // The 16-slot kernel's mirror is 8192 B per wavefront: 57344 B per workgroup allowed two workgroups per CU, 45056 B allow three
  // (and without the fp32 register copies it holds 159 VGPRs <= 168).
  constexpr bool HALF = !RAGGED && REGF && KMAX == 3 && FMAX == 16 && STD;
  constexpr int TILE_ROWS = HALF ? kWave / 2 : kWave;
  constexpr int TILE_FLOATS = TILE_ROWS * PITCH;
  // SUMMARY, register-food kernels: the env's record (32 B per lane) is kept in LDS behind the mirror and updated there every
  // step — these kernels sit at their register limits (eight more registers across the loop put 12-132 B of scratch into the
  // 4-slot ones, profiles/r06/ab_notes.md) and LDS limits none of them; the one-food kernels keep it in registers.
  constexpr bool EVLDS = SUMMARY && FMAX > 1;
  constexpr int EV_FLOATS = EVLDS ? kWave * SALP_EVAL_WORDS : 0;
  constexpr int WAVE_FLOATS = TILE_FLOATS + (REGF ? kWave * 2 * FMAX : 0) + EV_FLOATS;
  static_assert(!REGF || (4 * FMAX <= TILE_ROWS * PITCH && 96 <= TILE_ROWS * PITCH), "the placement's FMAX accepted points (16 B each) must fit in the tile");
  __shared__ __attribute__((aligned(16))) float lds[(kBlock / kWave) * WAVE_FLOATS];

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  // the wavefront number and everything derived from it (first env, row bases, tile address) as scalars: index
  // arithmetic then is a scalar base plus the lane, not 64-bit vector registers held across the loop
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t env0 = env_begin + (int64_t)blockIdx.x * kBlock + (int64_t)wave * kWave;  // first env of this wavefront
  const int64_t env = env0 + lane;
  const int rows = (int)((env_end - env0) < kWave ? ((env_end - env0) > 0 ? (env_end - env0) : 0) : kWave);
  const bool active = RAGGED ? (env < env_end) : true;     // !RAGGED: rows is 64 or 0
  // the env whose state the lane loads: its own — clamped into the range for the lanes past the end (RAGGED), or the
  // range's first wavefront for a whole wavefront past the end (!RAGGED; it runs no step and stores nothing)
  const int64_t envc = RAGGED ? ((env < env_end) ? env : (env_end - 1)) : ((rows > 0 ? env0 : env_begin) + lane);
  const uint64_t genv = P.env_base + (uint64_t)envc;
  const int K = (KMAX == 3) ? 3 : P.K;
  const int Q = 3 + K;
  const int OD = 4 * Q;
  const int AD = FORCED ? 1 : 2;
  float* tile = lds + wave * WAVE_FLOATS;
  float4* myrow4 = reinterpret_cast<float4*>(tile + (HALF ? (lane & (TILE_ROWS - 1)) : lane) * PITCH);
  // SWZ: column q of this lane's row sits at float4 (q ^ s), s = bit 2 of the row = q + s for even q, q - s for odd q
  const int swz = SWZ ? ((lane >> 2) & 1) : 0;
  float4* myrow_even = myrow4 + swz;
  float4* myrow_odd = myrow4 - swz;

  // Tile flush plan, fixed for the whole launch: float4 number f = j*64 + lane of the wavefront's
  // [rows x Q] tile lives at LDS row f / Q, column f % Q and goes to global float4 f of the run.
  int lds_off[QMAX];      // float offset inside the tile (-1: nothing to move, RAGGED only)
#pragma unroll
  for (int j = 0; j < QMAX; ++j) {
    const int f = j * kWave + lane;
    const int r = f / Q;
    const int c = f - r * Q;
    lds_off[j] = (!RAGGED || f < rows * Q) ? (r * PITCH + 4 * (SWZ ? (c ^ ((r >> 2) & 1)) : c)) : -1;
  }

  // the six source addresses of the flush as ONE register each: left to itself the compiler keeps the row term and
  // the swizzled column term of every address in separate registers and adds them on every step
  const v4f* flush_src[QMAX];
#pragma unroll
  for (int j = 0; j < QMAX; ++j) {
    int i = wave * WAVE_FLOATS + (lds_off[j] >= 0 ? lds_off[j] : 0);
    if constexpr ((!PACKED || TAILREG) && !SUMMARY) asm volatile("" : "+v"(i));
    flush_src[j] = reinterpret_cast<const v4f*>(lds + i);
  }
  // PACKED flush plan: float4 f = j*64 + lane of a tile pass (TILE_ROWS rows of TQ float4: Q + 1, TAILREG Q) lives at tile
  // row r = f / TQ, column c = f % TQ and goes to float4 r * RW4 + c of the pass's first record; RW4 = the record width in
  // float4 (Q + 1, or 2 Q + 1 with the terminal observation, which the flush skips).  Without the terminal observation the
  // wavefront's 64 records are one contiguous run and every store is a whole 1-KB line group, as in the other signatures.
  // The plan is kept as ONE byte per store — the row r, 0xFF: nothing to move (past the pass's last float4; RAGGED: a row
  // past the range) — four to a register, and both offsets are rebuilt from it at every flush (f + r * (pitch - TQ) in
  // the tile, f + r * (RW4 - TQ) in the block: a bit-field extract and a multiply-add per store).  An offset register per
  // store put the 8-, 12- and 16-slot kernels, which sit at their register limits, into scratch.
  constexpr int PJ = PACKED ? (TILE_ROWS * QPMAX + kWave - 1) / kWave : 1;
  const int NQ = Q + 1;
  const int TQ = TAILREG ? Q : NQ;
  const int RW4 = NQ + ((PACKED && io.final_obs) ? Q : 0);
  uint32_t rec_rows[(PJ + 3) / 4];
#pragma unroll
  for (int i = 0; i < (PJ + 3) / 4; ++i) rec_rows[i] = 0u;
#pragma unroll
  for (int j = 0; j < PJ; ++j) {
    const int f = j * kWave + lane;
    const int r = f / TQ;
    rec_rows[j >> 2] |= (uint32_t)((f < TILE_ROWS * TQ && (!RAGGED || r < rows)) ? r : 0xFF) << (8 * (j & 3));
  }
  // The record's last float4 waits in LDS from the step's end to the row writes (its values are those of BEFORE the
  // autoreset): 16 B per lane at tile bytes 384 .. 1407, which the rare paths leave alone (placement scratch 0 .. 255,
  // wave_stats 256 .. 383) and every tile covers (>= 3584 B) — not four registers across the rare region and observe().
  // (Not TAILREG: stored at once.)
  float4* const rec_stash = reinterpret_cast<float4*>(tile + 96) + lane;
  // Event statistics (episodes, terminations, food, ...) change on rare steps only: they are accumulated with LDS integer
  // atomics inside the rare-event branch — in 128 bytes of the wavefront's own tile, idle there — and leave with ONE
  // global atomic instruction per wavefront and event step, into one of 64 line-sized replicas.  (Rounds 1-2 kept a
  // 128-byte block of LDS per workgroup for the whole launch: with the mirror that was exactly what pushed the 8-slot
  // kernel from four workgroups per CU to three.)
  unsigned long long* const wave_stats = reinterpret_cast<unsigned long long*>(tile) + 32;   // tile bytes 256..383 (placement scratch: 0..191)
  DevStats* const stats_replica = io.stats ? io.stats + (blockIdx.x % SALP_STATS_REPLICAS) : nullptr;

  using EnvT = std::conditional_t<LDSF, EnvCore, Env<FMAX>>;
  EnvT e;
  const FoodLds food{food_lds + (LDSF ? (wave * FMAX * kWave + lane) : 0)};
  const MirrorLds mir{reinterpret_cast<float2*>(tile + TILE_FLOATS) + lane};   // REGF only
  FoodF32<REGF ? FMAX : 1, food_in_registers(FMAX, KMAX, STD, SIG == 1 || SIG == 4) && !HALF> ff;   // REGF: fp32 roundings of the food positions (salp_food_reg.h)
  FoodScan<KMAX> fq;          // MULTI: nearest-K selection of the current food set around the current pose
  int nlive = 0;              // MULTI: live foods of this env, recounted whenever the food set changes
  int order_cache = -1;       // REGF: remembered exact order of a resting swimmer's foods (step_env_reg)
  if constexpr (LDSF) {
    load_core(e, S, P, envc);
    for (int k = 0; k < P.F; ++k) {
      const double fx = S.f[(SF_FOOD0 + k) * P.pitch + envc];
      food.set(k, fx, S.f[(SF_FOOD0 + P.F + k) * P.pitch + envc]);
      nlive += is_none(fx) ? 0 : 1;
    }
    for (int k = P.F; k < FMAX; ++k) food.clear(k);   // the scans run over whole groups of four slots
  } else {
    load_env(e, S, P, envc);
    if constexpr (REGF) {
#pragma unroll
      for (int k = 0; k < FMAX; ++k) {
        nlive += is_none(e.fx[k]) ? 0 : 1;
        ff.set(k, e.fx[k], e.fy[k]);
        mir.set(k, e.fx[k], e.fy[k]);
      }
    }
  }

  double st_reward = 0.0;   // the one per-step statistic
  // SUMMARY: the env's record (include/salp_vec.h SALP_EVAL_*): two doubles and four ints per lane, in registers (one food)
  // or in the lane's own two float4 of LDS (EVLDS: float4 `lane` holds the sums, float4 `64 + lane` the counts — consecutive
  // lanes 16 B apart, conflict-free; only the lane itself ever touches them, so no barrier is involved)
  double ev_ret = 0.0, ev_first_ret = 0.0;
  int ev_first_len = 0, ev_first_end = 0, ev_episodes = 0, ev_food = 0;
  int4* const ev_lds = reinterpret_cast<int4*>(tile + WAVE_FLOATS - EV_FLOATS) + lane;
  // NAV: the env's record (include/salp_vec.h SALP_NAV_*) in registers, with the trial's line; `running` = the lane is stepped
  [[maybe_unused]] double nv_path = 0.0, nv_lat = 0.0, nv_xmin = 0.0, nv_xmax = 0.0, nv_ymin = 0.0, nv_ymax = 0.0;
  [[maybe_unused]] double nv_sx = 0.0, nv_sy = 0.0, nv_gx = 0.0, nv_gy = 0.0, nv_dnx = 0.0, nv_dny = 0.0;
  [[maybe_unused]] int nv_steps = 0, nv_status = 0, nv_steps0 = 0;
  [[maybe_unused]] bool running = true;
  if constexpr (NAV) {
    nv_xmin = nv_xmax = e.x; nv_ymin = nv_ymax = e.y;     // a fresh record: the box is the entry position
    if (rows > 0) {
      const double2* const lp2 = reinterpret_cast<const double2*>(io.nav_line) + envc * 2;
      const double2 s2 = lp2[0], g2 = lp2[1];
      nv_sx = s2.x; nv_sy = s2.y; nv_gx = g2.x; nv_gy = g2.y;
      const double dx = nv_gx - nv_sx, dy = nv_gy - nv_sy;
      const double L = sqrt(dx * dx + dy * dy) + 1e-12;
      nv_dnx = dx / L; nv_dny = dy / L;
      if (io.final_obs) {     // SALP_EVAL_ACCUMULATE: continue the caller's record unless it is a fresh one (steps == 0 && status == 0)
        const int4* const rp = reinterpret_cast<const int4*>(io.obs) + envc * (SALP_NAV_WORDS / 4);
        const int4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
        if (r0.x != 0 || r0.y != 0) {
          nv_steps = r0.x; nv_status = r0.y;
          nv_path = __hiloint2double(r0.w, r0.z);
          nv_lat = __hiloint2double(r1.y, r1.x);
          nv_xmin = __hiloint2double(r1.w, r1.z);
          nv_xmax = __hiloint2double(r2.y, r2.x);
          nv_ymin = __hiloint2double(r2.w, r2.z);
          nv_ymax = __hiloint2double(r3.y, r3.x);
        }
      }
    }
    nv_steps0 = nv_steps;
    running = active && rows > 0 && (nv_status & 1) == 0;
  }
  if constexpr (SUMMARY && !NAV) {
    int4 ra = make_int4(0, 0, 0, 0), rb = make_int4(0, 0, 0, 0);
    if (io.final_obs && rows > 0) {     // SALP_EVAL_ACCUMULATE: continue the caller's record (complete at the vmcnt(0) below)
      const int4* const rp = reinterpret_cast<const int4*>(io.obs) + envc * 2;
      ra = rp[0]; rb = rp[1];
    }
    if constexpr (EVLDS) {
      ev_lds[0] = ra; ev_lds[kWave] = rb;
    } else {
      ev_ret = __hiloint2double(ra.y, ra.x);
      ev_first_ret = __hiloint2double(ra.w, ra.z);
      ev_first_len = rb.x; ev_first_end = rb.y; ev_episodes = rb.z; ev_food = rb.w;
    }
  }

  float a0 = 0.f, a1 = 0.f;
  U4 aw0 = {0u, 0u, 0u, 0u}, aw1 = {0u, 0u, 0u, 0u};   // GEN: the current Philox block of each action component
  if (ACT == ACT_READ) {
    a0 = io.act[envc * AD];
    a1 = FORCED ? 0.f : io.act[envc * AD + 1];
  }
  uint32_t pol_off = 0u;    // POLICY: word offset of this wavefront's policy in the block (wave-uniform)
  [[maybe_unused]] uint32_t noise0 = 0u;   // SAMPLED: low word of the policy's noise step at entry (wave-uniform)
  [[maybe_unused]] float lp = 0.f;         // SAMPLED: log-probability of the action in a0 / a1
  if constexpr (POLICY) {
    if (rows > 0) {
      pol_int* const hd = (pol_int*)(uintptr_t)io.act;
      const uint32_t group = (uint32_t)hd[PH_GROUP], npol = (uint32_t)hd[PH_COUNT];
      uint32_t pi = (uint32_t)env0 / group;          // env i runs policy i / (n_envs / P)
      pi = pi < npol ? pi : npol - 1u;
      pol_off = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pi * (uint32_t)hd[PH_STRIDE]));
      if constexpr (SAMPLED) noise0 = (uint32_t)hd[PH_NOISE];
      // the env's current observation, as the end of a step forms it (below), from the loaded state: the SAME bits as the
      // row of the step that left this state, so that a rollout cut into several calls takes the actions of one call.
      // The one thing in a row that the state does not spell out is which bearing polynomial its nearest food went
      // through: the step hands the reward's own (PRECISE) bearing to the row (`have_rel`) unless the food set or the
      // episode changed behind it — per lane in the one-food kernels (a capture or an autoreset: both leave
      // steps_since_food == 0, which no other step does), for the whole wavefront in the register-food kernels (any lane
      // that captured or finished sends the wavefront through the rare region, which selects again for every lane;
      // `finished` is the step's own test on the state it left).  A state that no step left (reset, set_state) may
      // fall either way.
      double ea, eb;
      shape_of<STD>(P, e.packed, e.water, ea, eb);
      const double r0 = pymax(ea, eb);
      float ob0[12 + 4 * KMAX];
      if constexpr (REGF) {
        SALP_CONSTS;
        select_foods_reg<FMAX, KMAX, false, true>(e, ff, mir, K, (STD ? StdConsts::tie_c0 : P.tie_c0), fq, nlive);
        const double mg = CV(margin);
        const bool hit = (e.x - r0 <= mg) || (e.x + r0 >= CV(wall_hi_x)) || (e.y - r0 <= mg) || (e.y + r0 >= CV(wall_hi_y));
        const bool finished = hit || (e.ssf > P.max_steps_wo_food) || (!P.respawn && nlive == 0);
        const bool have_rel0 = !__any(e.ssf == 0 || finished) && (fq.idx[0] >= 0);
        const float rel0 = relative_heading<true>(fq.by[0], fq.bx[0], (float)e.th);
        observe_lds<KMAX, STD>(e, P, r0, K, fq, nlive, have_rel0, rel0, ob0);
      } else {
        bool have_rel0 = false;
        float rel0 = 0.f;
        if (P.prox_w > 0) {
          const Nearest g = nearest_food(e);
          if (g.any) {
            rel0 = relative_heading<true>((float)g.dy, (float)g.dx, (float)e.th);
            have_rel0 = e.ssf != 0;
          }
        }
        observe<FMAX, KMAX, STD>(e, P, r0, have_rel0, rel0, ob0);
      }
      if constexpr (SAMPLED) {
        const U4 nw = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), noise0, 3u, P.seed[0], P.seed[1]);
        policy_eval_impl<12 + 4 * KMAX, FORCED ? 1 : 2, true>(io.act, pol_off, ob0, a0, a1, policy_normal(nw.x, nw.y),
                                                               FORCED ? 0.f : policy_normal(nw.z, nw.w), lp);
      } else
      policy_eval<12 + 4 * KMAX, FORCED ? 1 : 2>(io.act, pol_off, ob0, a0, a1);
    }
  }
  // Everything loaded so far is complete before the loop is entered: otherwise the waitcnt pass keeps
  // a conservative `s_waitcnt vmcnt(1)` on the first use of the action inside the loop (for the entry
  // path), and that wait drains the previous step's stores on every iteration.
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)

  const int Hrun = (rows > 0) ? H : 0;   // a wavefront past the end of the range runs zero steps
#ifdef SALP_EXP_STAMPS
  StampAcc stamps;
  for (int i = 0; i < 12; ++i) stamps.acc[i] = 0u;
  stamps.last = (uint32_t)__builtin_amdgcn_s_memtime();
  StampAcc* const stamps_ = &stamps;
  const uint32_t stamp_real0 = (uint32_t)__builtin_amdgcn_s_memrealtime();   // 100 MHz: wall clock of the wavefront's loop
#endif
#pragma unroll 1
  for (int t = 0; t < Hrun; ++t) {
    const int64_t rowbase = (int64_t)t * P.n;
    float c0 = a0, c1 = a1;
    if constexpr (NAV) {
      if (!__any(running)) {     // every trial of the wavefront has ended: the remaining track rows repeat the last positions
        if (io.nav_track && active) {
#pragma unroll 1
          for (int u = t; u < Hrun; ++u) reinterpret_cast<double2*>(io.nav_track)[(int64_t)u * P.n + env] = make_double2(e.x, e.y);
        }
        break;
      }
    }
    [[maybe_unused]] const double nv_px = e.x, nv_py = e.y;     // NAV: the position before the step
    if (GEN) {
      // device action stream (include/salp_vec.h "Randomness"): word ts & 3 of block ts >> 2
      const uint32_t ts = (uint32_t)(io.global_step + t);
      if (t == 0 || (ts & 3u) == 0u) {   // wave-uniform
        aw0 = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), ts >> 2, 1u, P.seed[0], P.seed[1]);
        if (!FORCED) aw1 = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), ts >> 2, 2u, P.seed[0], P.seed[1]);
      }
      const uint32_t k = ts & 3u;
      const uint32_t w0 = (k == 0) ? aw0.x : (k == 1) ? aw0.y : (k == 2) ? aw0.z : aw0.w;
      if (FORCED) {
        c0 = (float)(w0 >> 8) * 1.1920928955078125e-7f - 1.0f;              // [-1, 1)
      } else {
        const uint32_t w1 = (k == 0) ? aw1.x : (k == 1) ? aw1.y : (k == 2) ? aw1.z : aw1.w;
        c0 = (float)(w0 >> 8) * 5.9604644775390625e-8f;                     // inhale control in [0, 1)
        c1 = (float)(w1 >> 8) * 1.1920928955078125e-7f - 1.0f;
      }
      if (io.act_out && active) {
        io.act_out[(rowbase + env) * AD] = c0;
        if (!FORCED) io.act_out[(rowbase + env) * AD + 1] = c1;
      }
    } else if (POLICY) {
      if (!SUMMARY && io.act_out && active) {
        io.act_out[(rowbase + env) * AD] = c0;
        if (!FORCED) io.act_out[(rowbase + env) * AD + 1] = c1;
      }
      if constexpr (SAMPLED && !SUMMARY) {
        if (io.logp_out && active) io.logp_out[rowbase + env] = lp;
      }
    } else {  // prefetch the next step's action (the last step re-reads its own: keeps the load unconditional)
      const int64_t nb = (rowbase + ((t + 1 < H) ? P.n : 0) + envc) * AD;
      a0 = io.act[nb];
      if (!FORCED) a1 = io.act[nb + 1];
    }

#ifdef SALP_EXP_STORE_ONLY   // experiment build: no simulation, only the output stream
    StepOut o; o.rmax = 30.0; o.reward = c0; o.rel = c1; o.rel_valid = true;
    o.terminated = o.truncated = o.collision = o.collected = false;
#else
    StepOut o;
    if constexpr (LDSF) o = step_env_lds<KMAX, FORCED, STD>(e, food, P, genv, c0, c1, K, fq, nlive);
    else if constexpr (REGF) {
#ifdef SALP_EXP_STAMPS
      { StampAcc* stamps_ = &stamps; SALP_STAMP(0); }
      o = step_env_reg<FMAX, KMAX, FORCED, STD>(e, ff, mir, P, genv, c0, c1, K, fq, nlive, order_cache, &cold->P, &stamps);
#else
      o = step_env_reg<FMAX, KMAX, FORCED, STD>(e, ff, mir, P, genv, c0, c1, K, fq, nlive, order_cache, &cold->P);
#endif
    }
    else if constexpr (NAV) {
      // only the running lanes are stepped; for the others `o` says that nothing happened, so the rare-event region below
      // (statistics, respawn) passes them by and their state keeps every bit
      o.rmax = 0.0; o.reward = 0.f; o.rel = 0.f; o.rel_valid = false;
      o.terminated = o.truncated = o.collision = o.collected = false;
      if (running) {
#ifdef SALP_EXP_STAMPS
        o = step_env<FMAX, FORCED, STD>(e, P, genv, c0, c1, &stamps);
#else
        o = step_env<FMAX, FORCED, STD>(e, P, genv, c0, c1);
#endif
      }
    }
    else {
#ifdef SALP_EXP_STAMPS
      { StampAcc* stamps_ = &stamps; SALP_STAMP(0); }
      o = step_env<FMAX, FORCED, STD>(e, P, genv, c0, c1, &stamps);
#else
      o = step_env<FMAX, FORCED, STD>(e, P, genv, c0, c1);
#endif
    }
#endif
    const bool done = o.terminated || o.truncated;
    double rmax = o.rmax;
    bool have_rel = o.rel_valid;

    // PACKED: the record's last float4, taken here (the values of the step's own episode, before the autoreset below)
    if constexpr (PACKED) {
      const uint32_t fl = (o.terminated ? 1u : 0u) | (o.truncated ? 0x100u : 0u) | (o.collision ? 0x10000u : 0u);
      const float4 last = make_float4(o.reward, __uint_as_float(fl), __uint_as_float((uint32_t)e.fc), __uint_as_float((uint32_t)e.ssf));
      if constexpr (TAILREG) reinterpret_cast<float4*>(io.obs)[(rowbase + env) * RW4 + Q] = last;
      else *rec_stash = last;
    }
    if (!PACKED && !SUMMARY && active) {
      // reward: one dword per lane (256 B per wavefront); flags: one byte per lane.  (Rebuilding the
      // 64 flag bytes from a ballot and storing 16 dwords was measured: no faster in the memory
      // pipeline and slower overall, profiles/r01/ab_notes.md.)
      // (cache-policy bits on these small stores, and issuing them after the rows: measured, slower — r02 sessions 11, 14, 15)
      if (FULL || io.reward) io.reward[rowbase + env] = o.reward;
      if (FULL || io.terminated) io.terminated[rowbase + env] = o.terminated ? 1 : 0;
      if (FULL || io.truncated) io.truncated[rowbase + env] = o.truncated ? 1 : 0;
      if (EXTRAS && io.info) {
        int32_t* ip = io.info + (rowbase + env) * SALP_INFO_COLS;
        ip[SALP_INFO_FOOD_COLLECTED] = e.fc;
        ip[SALP_INFO_STEPS_SINCE_FOOD] = e.ssf;
        ip[SALP_INFO_COLLISION] = o.collision ? 1 : 0;
      }
    }
    st_reward += (double)o.reward;
    if constexpr (NAV) {
      // the record of the step just taken, in fp64 with IEEE sqrt (include/salp_vec.h "Navigation evaluation": a host loop
      // reproduces every bit); a lane that reaches the goal stops running behind this step
      if (running) {
        const double x = e.x, y = e.y;
        const double sx_ = x - nv_px, sy_ = y - nv_py;
        nv_path += sqrt(sx_ * sx_ + sy_ * sy_);
        nv_lat += fabs((x - nv_sx) * nv_dny - (y - nv_sy) * nv_dnx);
        nv_xmin = fmin(nv_xmin, x); nv_xmax = fmax(nv_xmax, x);
        nv_ymin = fmin(nv_ymin, y); nv_ymax = fmax(nv_ymax, y);
        nv_steps += 1;
        nv_status |= (o.collision ? 2 : 0) | (o.collected ? 4 : 0);
        const double gx_ = x - nv_gx, gy_ = y - nv_gy;
        if (sqrt(gx_ * gx_ + gy_ * gy_) < io.nav_radius) { nv_status |= 1; running = false; }
      }
      // one 16-byte store per lane, 1 KB contiguous per wavefront; a stopped env repeats its last position
      if (io.nav_track && active) reinterpret_cast<double2*>(io.nav_track)[rowbase + env] = make_double2(e.x, e.y);
    } else
    if constexpr (SUMMARY) {    // the float32 reward a rollout would have stored, added in step order in fp64; nothing below changes these
      const double r64 = (double)o.reward;
      const int end_now = o.terminated ? 1 : (o.truncated ? 2 : 0);     // terminated wins, as in the statistics below
      if constexpr (EVLDS) {
        int4 sa = ev_lds[0], sb = ev_lds[kWave];
        const double ret = __hiloint2double(sa.y, sa.x) + r64;
        double first = __hiloint2double(sa.w, sa.z);
        const bool open = sb.y == 0;
        if (open) first += r64;
        sb.x += open ? 1 : 0;
        sb.y = open ? end_now : sb.y;
        sb.z += done ? 1 : 0;
        sb.w += o.collected ? 1 : 0;
        ev_lds[0] = make_int4(__double2loint(ret), __double2hiint(ret), __double2loint(first), __double2hiint(first));
        ev_lds[kWave] = sb;
      } else {
        ev_ret += r64;
        if (ev_first_end == 0) {
          ev_first_ret += r64;
          ev_first_len += 1;
          ev_first_end = end_now;
        }
        ev_episodes += done ? 1 : 0;
        ev_food += o.collected ? 1 : 0;
      }
    }

    SALP_STAMP(6);
    // rare events: respawn of a collected food (snake:179-180), then same-step autoreset
    int todo = (o.collected && P.respawn) ? 1 : 0;
    const int F_base = P.F_base;
#ifdef SALP_EXP_NO_RARE   // experiment build: price of the respawn / autoreset region (results are wrong)
    if (false) {
#else
    if (__any(o.collected || done)) {
#endif
      const DevParams& C = cold->P;   // rare path: constants from memory, not from scalar registers
      int limit = 50;
      if (o.collected || done) order_cache = -1;      // the food set (or the episode) changes
      if (io.stats) {
        if (lane < 16) wave_stats[lane] = 0ull;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (active) {
          if (o.collected) atomicAdd(&wave_stats[ST_FOOD], 1ull);
          if (o.collision) atomicAdd(&wave_stats[ST_COLL], 1ull);
          if (done && C.autoreset) {
            atomicAdd(&wave_stats[ST_EPISODES], 1ull);
            atomicAdd(&wave_stats[o.terminated ? ST_TERM : ST_TRUNC], 1ull);
            atomicAdd(&wave_stats[ST_EPLEN], (unsigned long long)e.eplen);
            atomicAdd(&wave_stats[ST_EPRET], (unsigned long long)__double2ll_rn(e.epret * SALP_FIXED_SCALE));
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane <= ST_EPRET) {
          const unsigned long long v = wave_stats[lane];
          if (v != 0) atomicAdd(&stats_replica->v[lane], v);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // the placement's scratch and the tile rows come next
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      SALP_STAMP(10);
#pragma unroll 1
      for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && done && C.autoreset) {
          if (EXTRAS && io.final_obs && active) {
            float fo[12 + 4 * KMAX];
            if constexpr (LDSF) {   // the terminal observation sees the respawned food (pass 0)
              bool c_; int h_;
              scan_foods<KMAX, false, true>(food, C.F, e.x, e.y, 0.0, fq, c_, h_, nlive);
              if (__any(fq.tie)) exact_order_lds<KMAX>(food, C.F, K, e.x, e.y, fq);
              resolve<KMAX>(food, K, e.x, e.y, fq);
              observe_lds<KMAX, STD>(e, C, rmax, K, fq, nlive, false, 0.f, fo);
            } else if constexpr (REGF) {
              select_foods_reg<FMAX, KMAX, false, true>(e, ff, mir, K, (STD ? StdConsts::tie_c0 : C.tie_c0), fq, nlive);
              observe_lds<KMAX, STD>(e, C, rmax, K, fq, nlive, false, 0.f, fo);
            } else {
              observe<FMAX, KMAX, STD>(e, C, rmax, have_rel, o.rel, fo);
            }
            float4* dst = PACKED ? reinterpret_cast<float4*>(io.obs) + (rowbase + env) * RW4 + NQ     // the record's own tail
                                 : reinterpret_cast<float4*>(io.final_obs + (rowbase + env) * OD);
#pragma unroll
            for (int q = 0; q < QMAX; ++q)
              if (q < Q) dst[q] = make_float4(fo[4 * q], fo[4 * q + 1], fo[4 * q + 2], fo[4 * q + 3]);
          }
          if constexpr (LDSF) {
            todo = reset_core<STD>(e, C, genv, F_base);
            for (int k = 0; k < C.F; ++k) food.clear(k);
          } else {
            todo = reset_pose<FMAX, STD>(e, C, genv, F_base);
            if constexpr (REGF) {
#pragma unroll
              for (int k = 0; k < FMAX; ++k) { ff.clear(k, true); mir.clear(k); }
            }
          }
          limit = 100;
          rmax = STD ? StdConsts::R : C.R;
          have_rel = false;
        }
        if constexpr (LDSF) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          place_food_coop<FMAX, STD>(e, food_lds + wave * FMAX * kWave, lane, C, genv, todo, limit);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        else if constexpr (REGF) place_food_coop_reg<FMAX, STD, food_in_registers(FMAX, KMAX, STD, SIG == 1 || SIG == 4) && !HALF>(e, ff, mir, lane, C, genv, todo, limit, reinterpret_cast<double2*>(tile));
        else place_food<FMAX, STD>(e, C, genv, todo, limit);
        todo = 0;
      }
      SALP_STAMP(11);
      if constexpr (LDSF) {   // the food set (or the pose) changed: select again for the observation
        bool c_; int h_;
        scan_foods<KMAX, false, true>(food, C.F, e.x, e.y, 0.0, fq, c_, h_, nlive);
        if (__any(fq.tie)) exact_order_lds<KMAX>(food, C.F, K, e.x, e.y, fq);
        resolve<KMAX>(food, K, e.x, e.y, fq);
        have_rel = false;
      }
      if constexpr (REGF) {   // likewise (the exact order's scratch and the placement's are the same idle tile bytes, used in turn)
        select_foods_reg<FMAX, KMAX, false, true>(e, ff, mir, K, (STD ? StdConsts::tie_c0 : C.tie_c0), fq, nlive);
        have_rel = false;
      }
    }
    SALP_STAMP(7);

    if (SUMMARY ? (t + 1 < Hrun) : (FULL || io.obs)) {     // SUMMARY: the row exists for the next action only
      float ob[12 + 4 * KMAX];
      if constexpr (REGF) {
        // all FMAX slots of every lane alive (the steady state with respawn) => every lane shows K foods
        if ((KMAX <= FMAX) && K >= 1 && __all(nlive == FMAX)) observe_lds<KMAX, STD, true>(e, P, rmax, K, fq, nlive, have_rel, o.rel, ob);
        else observe_lds<KMAX, STD>(e, P, rmax, K, fq, nlive, have_rel, o.rel, ob);
      } else if constexpr (LDSF) observe_lds<KMAX, STD>(e, P, rmax, K, fq, nlive, have_rel, o.rel, ob);
      else observe<FMAX, KMAX, STD>(e, P, rmax, have_rel, o.rel, ob);
      SALP_STAMP(8);
      // (per-lane 96-B rows stored straight from registers, without the LDS transpose: 2.1x slower, r01 ab_notes)
      [[maybe_unused]] v4f* gout = nullptr;
      if constexpr (!SUMMARY) gout = reinterpret_cast<v4f*>(io.obs + (rowbase + env0) * OD) + lane;
      if constexpr (SUMMARY) {
        // nothing is stored
      } else if constexpr (PACKED) {
        // the record rows through the tile, in one pass or (HALF) two of 32 rows; each pass is PJ 16-B-per-lane stores
        v4f* const rec0 = reinterpret_cast<v4f*>(io.obs) + (rowbase + env0) * RW4;
        const v4f* const tile4 = reinterpret_cast<const v4f*>(tile);
        const int skip4 = RW4 - TQ;                 // float4 the flush skips behind every tile row (wave-uniform)
#pragma unroll
        for (int i = 0; i < (PJ + 3) / 4; ++i) asm volatile("" : "+v"(rec_rows[i]));     // unpacked here, at every flush (see the plan)
        auto row_of = [&](int j) { return (int)((rec_rows[j >> 2] >> (8 * (j & 3))) & 0xFFu); };
        // whole store instructions of an unpredicated K = 3 launch carry no test at all
        auto moves = [&](int j) { return (!RAGGED && KMAX == 3 && (j + 1) * kWave <= TILE_ROWS * QPMAX) ? true : row_of(j) != 0xFF; };
        float4 tail = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (!TAILREG) {
          // every lane's, before ANY lane writes a row over the stash: the rows of other lanes cover it, which the compiler,
          // reasoning about one lane, cannot see — without the barrier it sank this read below the row writes
          tail = *rec_stash;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
#pragma unroll
        for (int h = 0; h < (HALF ? 2 : 1); ++h) {
          if (!HALF || (lane >> 5) == h) {
#pragma unroll
            for (int q = 0; q < QMAX; ++q)
              if (q < Q) ((q & 1) ? myrow_odd : myrow_even)[q] = make_float4(ob[4 * q], ob[4 * q + 1], ob[4 * q + 2], ob[4 * q + 3]);
            if constexpr (!TAILREG) myrow4[Q] = tail;
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          v4f tv[PJ];
#pragma unroll
          for (int j = 0; j < PJ; ++j)
            if (moves(j)) {
              if constexpr (TAILREG) tv[j] = *flush_src[j];        // the swizzled six-column tile of the unpacked signatures
              else tv[j] = tile4[j * kWave + lane + row_of(j) * (PITCH / 4 - TQ)];
            }
          v4f* const pass0 = rec0 + h * TILE_ROWS * RW4;
#pragma unroll
          for (int j = 0; j < PJ; ++j)
            if (moves(j)) __builtin_nontemporal_store(tv[j], &pass0[j * kWave + lane + row_of(j) * skip4]);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // this pass's reads before the next writes of the tile
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
      } else if constexpr (HALF) {
        // float4 f = j*64 + lane (j = 0..2) of a half lives at tile row f / 6, column f % 6 (flush_src[0..2]) and goes to global
        // float4 (3 h + j) * 64 + lane of the wavefront's 64-row block: the same 1-KB stores as the full plan, three per half
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if ((lane >> 5) == h) {
#pragma unroll
            for (int q = 0; q < QMAX; ++q)
              ((q & 1) ? myrow_odd : myrow_even)[q] = make_float4(ob[4 * q], ob[4 * q + 1], ob[4 * q + 2], ob[4 * q + 3]);
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          v4f tv[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) tv[j] = *flush_src[j];
#pragma unroll
          for (int j = 0; j < 3; ++j) __builtin_nontemporal_store(tv[j], &gout[(3 * h + j) * kWave]);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // the reads of this half before the writes of the next
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
      } else {
#pragma unroll
      for (int q = 0; q < QMAX; ++q)   // 16-B LDS stores, conflict-free (see the tile layout above)
        if (q < Q) ((q & 1) ? myrow_odd : myrow_even)[q] = make_float4(ob[4 * q], ob[4 * q + 1], ob[4 * q + 2], ob[4 * q + 3]);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      {
        v4f tv[QMAX];
#pragma unroll
        for (int j = 0; j < QMAX; ++j)
          if (j < Q && (!RAGGED || lds_off[j] >= 0)) tv[j] = *flush_src[j];
        // Write-once stream far larger than L2 / Infinity Cache.  The unpredicated one-food K = 3 kernels issue the row stores
        // as `global_store_dwordx4 ... sc1 nt` — system scope (written through, not retained in L2) plus the
        // streaming hint: measured -4.2 % on the one-food kernel against `nt` alone, which is what
        // __builtin_nontemporal_store emits and what was -2.4 % against plain stores (profiles/r02/ab_notes.md
        // session 14).  The compiler has no builtin for the scope bits of a plain global store, hence the asm; its
        // waitcnt pass does not count these stores, which is safe: vmcnt retires in order, so a wait computed
        // without them can only wait longer, and nothing reads the stream back.  The hazard recogniser does not see
        // them either: gfx9 wants one wait state between a store of more than 64 bits and a VALU write of its data
        // registers, so the last store carries an `s_nop 0` (the end-of-step drain below follows anyway: !MULTI).
        if constexpr (!RAGGED && QMAX == 6 && !MULTI) {   // the write-bound one-food kernel; the VALU-bound multi-food ones: +1 %, not used
          v4f* const gout4 = gout + 4 * kWave;     // the instruction's immediate offset reaches 4095 B: two bases
#pragma unroll
          for (int j = 0; j < QMAX - 1; ++j)
            asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1 nt"
                         :: "v"(j < 4 ? gout : gout4), "v"(tv[j]), "n"((j & 3) * kWave * 16) : "memory");
          asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1 nt\n\ts_nop 0"
                       :: "v"(gout4), "v"(tv[QMAX - 1]), "n"(((QMAX - 1) & 3) * kWave * 16) : "memory");
        } else
#pragma unroll
        for (int j = 0; j < QMAX; ++j)
          if (j < Q && (!RAGGED || lds_off[j] >= 0)) __builtin_nontemporal_store(tv[j], &gout[j * kWave]);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      // the next step's action from this step's row, while the row stores are in flight (the last step needs none)
      if constexpr (POLICY) {
        if constexpr (SAMPLED) {
          if (SUMMARY || t + 1 < Hrun) {
            const U4 nw = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), noise0 + (uint32_t)(t + 1), 3u, P.seed[0], P.seed[1]);
            policy_eval_impl<12 + 4 * KMAX, FORCED ? 1 : 2, true>(io.act, pol_off, ob, a0, a1, policy_normal(nw.x, nw.y),
                                                                   FORCED ? 0.f : policy_normal(nw.z, nw.w), lp);
          }
        } else
        if (SUMMARY || t + 1 < Hrun) policy_eval<12 + 4 * KMAX, FORCED ? 1 : 2>(io.act, pol_off, ob, a0, a1);
      }
    }
    // One-food kernel (write-bound): drain this step's stores before the next step.  Measured
    // (profiles/r01/ab_notes.md): letting stores run ahead (vmcnt(9)) is 2-6 % SLOWER than draining —
    // wavefronts that stay in step keep the write stream of all CUs inside one contiguous [N x 96 B] slab
    // at a time.  The multi-food kernels are issue-bound at 2 wavefronts per SIMD: there the drain is a
    // stall nothing hides (-6.4 % without it, profiles/r02/ab_notes.md session 2).
    if constexpr (!MULTI && !SUMMARY) __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)   (SUMMARY: the loop has no store to drain)
    SALP_STAMP(9);
  }
#ifdef SALP_EXP_STAMPS
  if (lane == 0 && rows > 0) {
    const int gw = (int)((env0 - env_begin) / kWave) & (kStampWaves - 1);
    for (int i = 0; i < 12; ++i) salp_stamp_out[gw * 16 + i] = stamps.acc[i];
    salp_stamp_out[gw * 16 + 12] = stamp_real0;                                           // start (10-ns ticks, low word)
    salp_stamp_out[gw * 16 + 13] = (uint32_t)__builtin_amdgcn_s_memrealtime();            // end
  }
#endif

  if (rows > 0 && active) {
    const DevParams& C = cold->P;
    const DevState CS = cold->S;
    if constexpr (LDSF) {
      store_core(e, CS, C, env);
      for (int k = 0; k < C.F; ++k) {
        double fx, fy;
        food.get(k, fx, fy);
        CS.f[(SF_FOOD0 + k) * C.pitch + env] = fx;
        CS.f[(SF_FOOD0 + C.F + k) * C.pitch + env] = fy;
      }
    } else {
      store_env(e, CS, C, env);
    }
    if constexpr (NAV) {         // the env's record: five 16-byte stores (a lane that took no step writes back what it read)
      int4* const rp = reinterpret_cast<int4*>(io.obs) + env * (SALP_NAV_WORDS / 4);
      rp[0] = make_int4(nv_steps, nv_status, __double2loint(nv_path), __double2hiint(nv_path));
      rp[1] = make_int4(__double2loint(nv_lat), __double2hiint(nv_lat), __double2loint(nv_xmin), __double2hiint(nv_xmin));
      rp[2] = make_int4(__double2loint(nv_xmax), __double2hiint(nv_xmax), __double2loint(nv_ymin), __double2hiint(nv_ymin));
      rp[3] = make_int4(__double2loint(nv_ymax), __double2hiint(nv_ymax), __double2loint(e.x), __double2hiint(e.x));
      rp[4] = make_int4(__double2loint(e.y), __double2hiint(e.y), 0, 0);
    } else
    if constexpr (SUMMARY) {     // the env's record: two 16-byte stores
      int4* const rp = reinterpret_cast<int4*>(io.obs) + env * 2;
      if constexpr (EVLDS) {
        rp[0] = ev_lds[0];
        rp[1] = ev_lds[kWave];
      } else {
        rp[0] = make_int4(__double2loint(ev_ret), __double2hiint(ev_ret), __double2loint(ev_first_ret), __double2hiint(ev_first_ret));
        rp[1] = make_int4(ev_first_len, ev_first_end, ev_episodes, ev_food);
      }
    }
  }

  if (io.stats) {
    // reward sum and env-step count: wavefront shuffles, the four wavefronts' sums through 64 bytes of the (now idle)
    // first tile, then two 64-bit integer global atomics per WORKGROUP (per wavefront they cost the H = 1 step kernel 8 %:
    // 8192 atomics on a 14-us launch, profiles/r03/ab_notes.md session 10)
    if (!active || rows == 0) st_reward = 0.0;
    const double wr = wave_sum(st_reward);
    // NAV: the steps the lanes actually took (a stopped env takes none)
    const int wact = wave_sum((active && rows > 0) ? (NAV ? nv_steps - nv_steps0 : 1) : 0);
    unsigned long long* const blk = reinterpret_cast<unsigned long long*>(lds);
    __syncthreads();                               // every wavefront is past its last tile flush
    if (lane == 0) {
      blk[2 * wave] = (unsigned long long)__double2ll_rn(wr * SALP_FIXED_SCALE);
      blk[2 * wave + 1] = (unsigned long long)((long long)wact * (NAV ? 1 : H));
    }
    __syncthreads();
    if (tid < 2) {
      unsigned long long v = 0ull;
      for (int w = 0; w < kBlock / kWave; ++w) v += blk[2 * w + tid];
      if (v != 0) atomicAdd(&stats_replica->v[tid == 0 ? ST_REWARD : ST_STEPS], v);
    }
  }
}

typedef void (*rollout_fn)(DevParams, DevState, IOPtrs, int, int64_t, int64_t, const ColdBlock*);

// Output signatures (template parameter SIG): kSigMain = obs, reward, terminated, truncated and nothing else — every
// store of the step loop is unconditional, so the compiler can count the stores issued after the action prefetch and wait
// for the prefetch alone; kSigExtras = the same four plus final_obs and / or info (salp_vec_step, rollouts that keep the
// terminal observations): the four main streams stay unconditional, only the extras are tested (the terminal rows are
// written in the rare-event region, the three info words per step); kSigPartial = some main output is NULL: every
// store is tested, the step ends in a full drain (a 12-food rollout with final_obs ran 22 % slower in that form,
// profiles/r03/ab_notes.md session 15).  The one-wavefront predicated launches exist as kSigMain and kSigPartial only.
// kSigPacked = ONE stream of transition records (salp_vec_step_packed / salp_vec_rollout_packed): no per-lane reward / flag /
// info stores at all; unpredicated and predicated, K = 3 and generic K; no in-kernel action generation.
// kSigSummary = NO per-step output: one record of SALP_EVAL_WORDS words per env at the end of the launch
// (salp_vec_evaluate_policy); exists for the in-kernel policy and K = 3 only, unpredicated and predicated.
// kSigNav = the summary kernel's loop with a per-env stop at a goal and one navigation record of SALP_NAV_WORDS words per env
// (salp_vec_evaluate_navigation); exists for one food, K = 3, forced breathing and the deterministic in-kernel policy only —
// four kernels, in the two one-food units.  Asked of anything else the choice is empty (fn NULL): the host refuses first.
enum { kSigPartial = 0, kSigMain = 1, kSigExtras = 2, kSigPacked = 3, kSigSummary = 4, kSigNav = 5 };
#ifdef SALP_EXP_STAMPS
// experiment build only: the per-wavefront phase cycle sums of this unit's last rollout launches (16 words per wavefront)
int exp_read_stamps(uint32_t* dst, int words) {
  const size_t n = sizeof(uint32_t) * (size_t)(words < kStampWaves * 16 ? words : kStampWaves * 16);
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(salp_stamp_out), n, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
#ifdef SALP_EXP_COUNT
int exp_read_counters(unsigned long long* dst) {
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(salp_exp_counter), 8 * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
template <int FMAX, int KMAX, bool FORCED, bool STD, int SIG, bool RAGGED, int ACT>
RolloutPick picked() {
  RolloutPick p = {};
  p.fn = (const void*)(rollout_fn)salp_rollout_kernel<FMAX, KMAX, FORCED, STD, SIG, RAGGED, ACT>;
  p.sig = SIG;
#ifdef SALP_EXP_STAMPS
  p.read_stamps = exp_read_stamps;
#endif
#ifdef SALP_EXP_COUNT
  p.read_counters = exp_read_counters;
#endif
  return p;
}
template <int FMAX, int KMAX, bool FORCED, bool STD, bool RAGGED, int ACT>
RolloutPick pick_sig(int sig) {
  if constexpr (ACT == ACT_POLICY || ACT == ACT_POLICY_SAMPLED) {
    if (sig == kSigNav) {
      if constexpr (ACT == ACT_POLICY && FMAX == 1 && KMAX == 3 && FORCED) return picked<FMAX, KMAX, FORCED, STD, kSigNav, RAGGED, ACT>();
      else return RolloutPick{nullptr, -1};
    }
    if (sig == kSigSummary) return picked<FMAX, KMAX, FORCED, STD, kSigSummary, RAGGED, ACT>();
    return picked<FMAX, KMAX, FORCED, STD, kSigMain, RAGGED, ACT>();
  } else if constexpr (ACT != ACT_READ) return picked<FMAX, KMAX, FORCED, STD, kSigMain, RAGGED, ACT>();
  else {
    if (sig == kSigMain) return picked<FMAX, KMAX, FORCED, STD, kSigMain, RAGGED, ACT_READ>();
    if (sig == kSigPacked) return picked<FMAX, KMAX, FORCED, STD, kSigPacked, RAGGED, ACT_READ>();
    if constexpr (!RAGGED)
      if (sig == kSigExtras) return picked<FMAX, KMAX, FORCED, STD, kSigExtras, false, ACT_READ>();
    return picked<FMAX, KMAX, FORCED, STD, kSigPartial, RAGGED, ACT_READ>();
  }
}
// `act`: where the actions come from (ACT_READ / ACT_GEN / ACT_POLICY / ACT_POLICY_SAMPLED)
template <int FMAX, int KMAX, bool STD, bool RAGGED>
RolloutPick pick_rollout(bool forced, int sig, int act) {
  if ((sig == kSigMain || sig == kSigSummary) && act == ACT_POLICY_SAMPLED)   // the same two signatures, sampling
    return forced ? pick_sig<FMAX, KMAX, true, STD, RAGGED, ACT_POLICY_SAMPLED>(sig) : pick_sig<FMAX, KMAX, false, STD, RAGGED, ACT_POLICY_SAMPLED>(sig);
  if ((sig == kSigMain || sig == kSigSummary || sig == kSigNav) && act == ACT_POLICY)   // the in-kernel policy exists for the main-only output signature and for the summary
    return forced ? pick_sig<FMAX, KMAX, true, STD, RAGGED, ACT_POLICY>(sig) : pick_sig<FMAX, KMAX, false, STD, RAGGED, ACT_POLICY>(sig);
  if (sig == kSigMain && act == ACT_GEN)
    return forced ? pick_sig<FMAX, KMAX, true, STD, RAGGED, ACT_GEN>(sig) : pick_sig<FMAX, KMAX, false, STD, RAGGED, ACT_GEN>(sig);
  return forced ? pick_sig<FMAX, KMAX, true, STD, RAGGED, ACT_READ>(sig) : pick_sig<FMAX, KMAX, false, STD, RAGGED, ACT_READ>(sig);
}
// The body of a K = 3 unit: both launch forms of one food-slot count and one kind of constants.
template <int FMAX, bool STD>
RolloutPick pick_k3(bool ragged, bool forced, int sig, int act) {
  return ragged ? pick_rollout<FMAX, 3, STD, true>(forced, sig, act) : pick_rollout<FMAX, 3, STD, false>(forced, sig, act);
}

}  // namespace
