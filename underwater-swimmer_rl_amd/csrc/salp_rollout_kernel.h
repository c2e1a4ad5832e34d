// salp_rollout_kernel.h — the fused SALP step/rollout kernel for gfx950 and the choice among its instantiations.
//
// Kernel design:
//   * one SALP per lane, 256-thread workgroups (4 wavefronts), env index = blockIdx*256 + tid;
//   * state is struct-of-arrays in HBM (row-major [quantity][env], 8-byte and 4-byte rows), read
//     once at kernel entry, held in VGPRs across the `horizon` steps, written once at exit;
//   * per step each wavefront stages its 64 observation rows (64 x obs_dim floats) in its private
//     LDS tile and streams them out as whole 16-byte-per-lane coalesced stores, so the
//     [horizon][n_envs][obs_dim] row-major output is written as contiguous 64*obs_dim*4-byte
//     runs per wavefront; actions are prefetched one step ahead, generated in the kernel, or computed by an in-kernel
//     policy from the row just written;
//   * the reward sum and the step count are reduced with wavefront shuffles and leave as two 64-bit integer atomics per
//     workgroup; the event statistics (episodes, terminations, food, ...) are counted in LDS on the rare steps that change
//     them and leave as one atomic instruction per wavefront and event step; both go to one of 64 line-sized replicas
//     (order-independent).
// MFMA in one place: the wide in-kernel policy (ACT_POLICY_WIDE*, salp_policy_wide.h), the path's one dense contraction,
// in the one-food kernels; everything else has none and its bound is HBM write bandwidth.
//
// Two headers: salp_rollout_traits.h — the launch arguments (IOPtrs, ColdBlock, the named meanings of IOPtrs' overloaded
// slots) and RolloutTraits, every compile-time switch and size of an instantiation with the reason for each and its LDS bytes
// pinned to the table of DESIGN.md §3.1;  this file — the kernel and the choice among its instantiations.  The kernel's body
// is still ONE function: each piece of it that was moved into a force-inlined function of its own changed the machine code
// of kernels that the move did not concern (the compiler optimises such a function on its own before it inlines it), most of
// them their register counts; profiles/r10/refactor_notes.md lists what was tried.  Its sections are marked `// ----`.
//
// The template is instantiated implicitly, by the small salp_rollout_*.hip units next to this file: one per food-slot count
// and literal / run-time constants for K = 3, one for the generic-K kernels, so that the 492 instantiations (52 of them the wide
// policy's, in the two one-food units) compile in parallel.  Each unit defines the rollout_unit_fn of its handle class (the generic unit: of its two); salp_vec.hip (the
// service kernels and the C ABI of include/salp_vec.h) reaches the kernels only through those.  No instantiation may be
// named in two units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>

#include <type_traits>

#include "salp_rollout_traits.h"
#include "salp_food_lds.h"
#include "salp_policy.h"
#include "salp_policy_wide.h"

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

// ---- experiment builds: what they put into the kernel, as one-line macros (no product build expands one to code) ----
// -DSALP_EXP_STAMPS: the wavefront's phase stamps (salp_exp.h SALP_STAMP) are opened before the step loop, handed to the
// step with SALP_STAMP_PASS and written out behind the loop.
#ifdef SALP_EXP_STAMPS
constexpr int kStampWaves = 8192;
__device__ uint32_t salp_stamp_out[kStampWaves * 16];
__device__ __forceinline__ uint32_t stamps_open(StampAcc& stamps) {
  for (int i = 0; i < 12; ++i) stamps.acc[i] = 0u;
  stamps.last = (uint32_t)__builtin_amdgcn_s_memtime();
  return (uint32_t)__builtin_amdgcn_s_memrealtime();   // 100 MHz: wall clock of the wavefront's loop
}
__device__ __forceinline__ void stamps_close(const StampAcc& stamps, uint32_t real0, bool first_lane, int64_t wave_index) {
  if (first_lane) {
    const int gw = (int)wave_index & (kStampWaves - 1);
    for (int i = 0; i < 12; ++i) salp_stamp_out[gw * 16 + i] = stamps.acc[i];
    salp_stamp_out[gw * 16 + 12] = real0;                                              // start (10-ns ticks, low word)
    salp_stamp_out[gw * 16 + 13] = (uint32_t)__builtin_amdgcn_s_memrealtime();         // end
  }
}
#define SALP_STAMPS_OPEN StampAcc stamps; const uint32_t stamp_real0 = stamps_open(stamps); StampAcc* const stamps_ = &stamps
#define SALP_STAMPS_CLOSE(first_lane, wave_index) stamps_close(stamps, stamp_real0, first_lane, wave_index)
#else
#define SALP_STAMPS_OPEN do {} while (0)
#define SALP_STAMPS_CLOSE(first_lane, wave_index) do {} while (0)
#endif
// -DSALP_EXP_STORE_ONLY: no simulation, only the output stream.  -DSALP_EXP_NO_RARE: the price of the respawn / autoreset
// region (results are wrong).
#ifdef SALP_EXP_STORE_ONLY
constexpr bool kExpStoreOnly = true;
#else
constexpr bool kExpStoreOnly = false;
#endif
#ifdef SALP_EXP_NO_RARE
#define SALP_RARE_TAKEN(cond) false
#else
#define SALP_RARE_TAKEN(cond) __any(cond)
#endif

// The kernel's action variables from the array that policy_eval (salp_policy.h) fills.  A function, not two assignments,
// on purpose: a0 and a1 then stay address-taken until the inliner has run, as they were when policy_eval took them by
// reference, and the kernels keep the order of their loop-carried values and with it their machine code
// (profiles/robot_rollout_notes.md "One evaluation function").
template <int AD>
__device__ __forceinline__ void take_actions(const float (&av)[AD], float& a0, float& a1) {
  a0 = av[0];
  if (AD == 2) a1 = av[1];
}

// The kernel.  What each switch of T means, and why it has its value: RolloutTraits (salp_rollout_traits.h).  The order of
// events: the launch geometry, the tile and its flush plan; load the state; load the record (SUMMARY / NAV); the first action;
// the loop — action, step, per-step outputs, record update, rare region, observation, flush, next action; store the state and
// the record; the launch statistics.
template <int FMAX, int KMAX, bool FORCED, bool STD, int SIG, bool RAGGED, int ACT>
__global__ __launch_bounds__(kBlock, (RolloutTraits<FMAX, KMAX, FORCED, STD, SIG, RAGGED, ACT>::waves_per_simd())) void salp_rollout_kernel(DevParams P_arg, DevState S, IOPtrs io, int H, int64_t env_begin, int64_t env_end, const ColdBlock* __restrict__ cold) {
  using T = RolloutTraits<FMAX, KMAX, FORCED, STD, SIG, RAGGED, ACT>;
  DevParams P_pol = P_arg;
  P_pol.use_mem = T::MEMC ? 1 : 0;
  const DevParams& P = STD ? P_arg : P_pol;
  double2* food_lds = nullptr;
  if constexpr (T::LDSF) {     // (declared only where it exists: a one-element stand-in would cost the 8-slot kernel its fourth workgroup per CU)
    __shared__ __attribute__((aligned(16))) double2 food_lds_block[T::FOOD_LDS_BYTES / sizeof(double2)];
    food_lds = food_lds_block;
  }
  __shared__ __attribute__((aligned(16))) float lds[(kBlock / kWave) * T::WAVE_FLOATS];

  // ---- the launch geometry
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
  float* tile = lds + wave * T::WAVE_FLOATS;
  float4* myrow4 = reinterpret_cast<float4*>(tile + (T::HALF ? (lane & (T::TILE_ROWS - 1)) : lane) * T::PITCH);
  // SWZ: column q of this lane's row sits at float4 (q ^ s), s = bit 2 of the row = q + s for even q, q - s for odd q
  const int swz = T::SWZ ? ((lane >> 2) & 1) : 0;
  float4* myrow_even = myrow4 + swz;
  float4* myrow_odd = myrow4 - swz;

  // ---- the tile's flush plan
  // Tile flush plan, fixed for the whole launch: float4 number f = j*64 + lane of the wavefront's
  // [rows x Q] tile lives at LDS row f / Q, column f % Q and goes to global float4 f of the run.
  int lds_off[T::QMAX];      // float offset inside the tile (-1: nothing to move, RAGGED only)
#pragma unroll
  for (int j = 0; j < T::QMAX; ++j) {
    const int f = j * kWave + lane;
    const int r = f / Q;
    const int c = f - r * Q;
    lds_off[j] = (!RAGGED || f < rows * Q) ? (r * T::PITCH + 4 * (T::SWZ ? (c ^ ((r >> 2) & 1)) : c)) : -1;
  }

  // the six source addresses of the flush as ONE register each: left to itself the compiler keeps the row term and
  // the swizzled column term of every address in separate registers and adds them on every step
  const v4f* flush_src[T::QMAX];
#pragma unroll
  for (int j = 0; j < T::QMAX; ++j) {
    int i = wave * T::WAVE_FLOATS + (lds_off[j] >= 0 ? lds_off[j] : 0);
    if constexpr ((!T::PACKED || T::TAILREG) && !T::SUMMARY) asm volatile("" : "+v"(i));
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
    const int NQ = Q + 1;
  const int TQ = T::TAILREG ? Q : NQ;
  const int RW4 = NQ + ((T::PACKED && packed_has_final(io)) ? Q : 0);
  uint32_t rec_rows[(T::PJ + 3) / 4];
#pragma unroll
  for (int i = 0; i < (T::PJ + 3) / 4; ++i) rec_rows[i] = 0u;
#pragma unroll
  for (int j = 0; j < T::PJ; ++j) {
    const int f = j * kWave + lane;
    const int r = f / TQ;
    rec_rows[j >> 2] |= (uint32_t)((f < T::TILE_ROWS * TQ && (!RAGGED || r < rows)) ? r : 0xFF) << (8 * (j & 3));
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

  // ---- load the state
  using EnvT = std::conditional_t<T::LDSF, EnvCore, Env<FMAX>>;
  EnvT e;
  const FoodLds food{food_lds + (T::LDSF ? (wave * FMAX * kWave + lane) : 0)};
  const MirrorLds mir{reinterpret_cast<float2*>(tile + T::TILE_FLOATS) + lane};   // REGF only
  FoodF32<T::REGF ? FMAX : 1, T::FOODREGS> ff;   // REGF: fp32 roundings of the food positions (salp_food_reg.h)
  FoodScan<KMAX> fq;          // MULTI: nearest-K selection of the current food set around the current pose
  int nlive = 0;              // MULTI: live foods of this env, recounted whenever the food set changes
  int order_cache = -1;       // REGF: remembered exact order of a resting swimmer's foods (step_env_reg)
  if constexpr (T::LDSF) {
    load_core(e, S, P, envc);
    for (int k = 0; k < P.F; ++k) {
      const double fx = S.f[(SF_FOOD0 + k) * P.pitch + envc];
      food.set(k, fx, S.f[(SF_FOOD0 + P.F + k) * P.pitch + envc]);
      nlive += is_none(fx) ? 0 : 1;
    }
    for (int k = P.F; k < FMAX; ++k) food.clear(k);   // the scans run over whole groups of four slots
  } else {
    load_env(e, S, P, envc);
    if constexpr (T::REGF) {
#pragma unroll
      for (int k = 0; k < FMAX; ++k) {
        nlive += is_none(e.fx[k]) ? 0 : 1;
        ff.set(k, e.fx[k], e.fy[k]);
        mir.set(k, e.fx[k], e.fy[k]);
      }
    }
  }

  // ---- load the record (SUMMARY / NAV)
  double st_reward = 0.0;   // the one per-step statistic
  // SUMMARY: the env's record (include/salp_vec.h SALP_EVAL_*): two doubles and four ints per lane, in registers (one food)
  // or in the lane's own two float4 of LDS (EVLDS: float4 `lane` holds the sums, float4 `64 + lane` the counts — consecutive
  // lanes 16 B apart, conflict-free; only the lane itself ever touches them, so no barrier is involved)
  double ev_ret = 0.0, ev_first_ret = 0.0;
  int ev_first_len = 0, ev_first_end = 0, ev_episodes = 0, ev_food = 0;
  int4* const ev_lds = reinterpret_cast<int4*>(tile + T::WAVE_FLOATS - T::EV_FLOATS) + lane;
  // NAV: the env's record (include/salp_vec.h SALP_NAV_*) in registers, with the trial's line; `running` = the lane is stepped
  [[maybe_unused]] double nv_path = 0.0, nv_lat = 0.0, nv_xmin = 0.0, nv_xmax = 0.0, nv_ymin = 0.0, nv_ymax = 0.0;
  [[maybe_unused]] double nv_sx = 0.0, nv_sy = 0.0, nv_gx = 0.0, nv_gy = 0.0, nv_dnx = 0.0, nv_dny = 0.0;
  [[maybe_unused]] int nv_steps = 0, nv_status = 0, nv_steps0 = 0;
  [[maybe_unused]] bool running = true;
  if constexpr (T::NAV) {
    nv_xmin = nv_xmax = e.x; nv_ymin = nv_ymax = e.y;     // a fresh record: the box is the entry position
    if (rows > 0) {
      const double2* const lp2 = reinterpret_cast<const double2*>(io.nav_line) + envc * 2;
      const double2 s2 = lp2[0], g2 = lp2[1];
      nv_sx = s2.x; nv_sy = s2.y; nv_gx = g2.x; nv_gy = g2.y;
      const double dx = nv_gx - nv_sx, dy = nv_gy - nv_sy;
      const double L = sqrt(dx * dx + dy * dy) + 1e-12;
      nv_dnx = dx / L; nv_dny = dy / L;
      if (accumulate(io)) {     // SALP_EVAL_ACCUMULATE: continue the caller's record unless it is a fresh one (steps == 0 && status == 0)
        const int4* const rp = reinterpret_cast<const int4*>(record_block(io)) + envc * (SALP_NAV_WORDS / 4);
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
  if constexpr (T::SUMMARY && !T::NAV) {
    int4 ra = make_int4(0, 0, 0, 0), rb = make_int4(0, 0, 0, 0);
    if (accumulate(io) && rows > 0) {     // SALP_EVAL_ACCUMULATE: continue the caller's record (complete at the vmcnt(0) below)
      const int4* const rp = reinterpret_cast<const int4*>(record_block(io)) + envc * 2;
      ra = rp[0]; rb = rp[1];
    }
    if constexpr (T::EVLDS) {
      ev_lds[0] = ra; ev_lds[kWave] = rb;
    } else {
      ev_ret = __hiloint2double(ra.y, ra.x);
      ev_first_ret = __hiloint2double(ra.w, ra.z);
      ev_first_len = rb.x; ev_first_end = rb.y; ev_episodes = rb.z; ev_food = rb.w;
    }
  }

  // ---- the first action
  float a0 = 0.f, a1 = 0.f;
  U4 aw0 = {0u, 0u, 0u, 0u}, aw1 = {0u, 0u, 0u, 0u};   // GEN: the current Philox block of each action component
  if (ACT == ACT_READ) {
    a0 = io.act[envc * AD];
    a1 = FORCED ? 0.f : io.act[envc * AD + 1];
  }
  uint32_t pol_off = 0u;    // POLICY: word offset of this wavefront's policy in the block (wave-uniform)
  [[maybe_unused]] uint32_t noise0 = 0u;   // SAMPLED: low word of the policy's noise step at entry (wave-uniform)
  [[maybe_unused]] float lp = 0.f;         // SAMPLED: log-probability of the action in a0 / a1
  if constexpr (T::POLICY) {
    if (rows > 0) {
      pol_int* const hd = (pol_int*)(uintptr_t)io.act;     // ACT_POLICY*: io.act is the policy's device block (set_policy_block)
      const uint32_t group = (uint32_t)hd[PH_GROUP], npol = (uint32_t)hd[PH_COUNT];
      uint32_t pi = (uint32_t)env0 / group;          // env i runs policy i / (n_envs / P)
      pi = pi < npol ? pi : npol - 1u;
      pol_off = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pi * (uint32_t)hd[PH_STRIDE]));
      if constexpr (T::SAMPLED) noise0 = (uint32_t)hd[PH_NOISE];
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
      float ob0[T::OBS];
      if constexpr (T::REGF) {
        SALP_CONSTS;
        select_foods_reg<FMAX, KMAX, false, true>(e, ff, mir, K, (STD ? StdConsts::tie_c0 : P.tie_c0), fq, nlive);
        const double mg = CV(margin);
        const bool hit = (e.x - r0 <= mg) || (e.x + r0 >= CV(wall_hi_x)) || (e.y - r0 <= mg) || (e.y + r0 >= CV(wall_hi_y));
        const bool finished = hit || (e.ssf > P.max_steps_wo_food) || (!P.respawn && nlive == 0);
        const bool have_rel0 = !__any(e.ssf == 0 || finished) && (fq.idx[0] >= 0);
        const float rel0 = relative_heading<true>(fq.by[0], fq.bx[0], (float)e.th);
        observe_selected<KMAX, STD>(e, P, r0, K, fq, nlive, have_rel0, rel0, ob0);
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
      float av[AD];
      if constexpr (T::SAMPLED) {
        const U4 nw = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), noise0, 3u, P.seed[0], P.seed[1]);
        float zv[AD];
        zv[0] = policy_normal(nw.x, nw.y);
        if constexpr (!FORCED) zv[1] = policy_normal(nw.z, nw.w);
        if constexpr (T::WIDE) policy_eval_wide<AD, true>(io.act, pol_off, ob0, zv, av, lp);
        else
        policy_eval_sampled<T::OBS, AD>(io.act, pol_off, ob0, zv, av, lp);
      } else if constexpr (T::WIDE) {
        const float zv[AD] = {};
        float unused = 0.f;
        policy_eval_wide<AD, false>(io.act, pol_off, ob0, zv, av, unused);
      } else
      policy_eval<T::OBS, AD>(io.act, pol_off, ob0, av);
      take_actions(av, a0, a1);
    }
  }
  // Everything loaded so far is complete before the loop is entered: otherwise the waitcnt pass keeps
  // a conservative `s_waitcnt vmcnt(1)` on the first use of the action inside the loop (for the entry
  // path), and that wait drains the previous step's stores on every iteration.
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)

  // ---- the step loop
  const int Hrun = (rows > 0) ? H : 0;   // a wavefront past the end of the range runs zero steps
  SALP_STAMPS_OPEN;
#pragma unroll 1
  for (int t = 0; t < Hrun; ++t) {
    const int64_t rowbase = (int64_t)t * P.n;
    float c0 = a0, c1 = a1;
    if constexpr (T::NAV) {
      if (!__any(running)) {     // every trial of the wavefront has ended: the remaining track rows repeat the last positions
        if (io.nav_track && active) {
#pragma unroll 1
          for (int u = t; u < Hrun; ++u) reinterpret_cast<double2*>(io.nav_track)[(int64_t)u * P.n + env] = make_double2(e.x, e.y);
        }
        break;
      }
    }
    [[maybe_unused]] const double nv_px = e.x, nv_py = e.y;     // NAV: the position before the step
    // ---- this step's action (READ: the prefetch of the next)
    if (T::GEN) {
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
    } else if (T::POLICY) {
      if (!T::SUMMARY && io.act_out && active) {
        io.act_out[(rowbase + env) * AD] = c0;
        if (!FORCED) io.act_out[(rowbase + env) * AD + 1] = c1;
      }
      if constexpr (T::SAMPLED && !T::SUMMARY) {
        if (io.logp_out && active) io.logp_out[rowbase + env] = lp;
      }
    } else {  // prefetch the next step's action (the last step re-reads its own: keeps the load unconditional)
      const int64_t nb = (rowbase + ((t + 1 < H) ? P.n : 0) + envc) * AD;
      a0 = io.act[nb];
      if (!FORCED) a1 = io.act[nb + 1];
    }

    // ---- the step
    StepOut o;
    if constexpr (kExpStoreOnly) {
      o.rmax = 30.0; o.reward = c0; o.rel = c1; o.rel_valid = true;
      o.terminated = o.truncated = o.collision = o.collected = false;
    } else if constexpr (T::LDSF) o = step_env_lds<KMAX, FORCED, STD>(e, food, P, genv, c0, c1, K, fq, nlive);
    else if constexpr (T::REGF) {
      SALP_STAMP(0);
      o = step_env_reg<FMAX, KMAX, FORCED, STD>(e, ff, mir, P, genv, c0, c1, K, fq, nlive, order_cache, &cold->P SALP_STAMP_PASS);
    }
    else if constexpr (T::NAV) {
      // only the running lanes are stepped; for the others `o` says that nothing happened, so the rare-event region below
      // (statistics, respawn) passes them by and their state keeps every bit
      o.rmax = 0.0; o.reward = 0.f; o.rel = 0.f; o.rel_valid = false;
      o.terminated = o.truncated = o.collision = o.collected = false;
      if (running) o = step_env<FMAX, FORCED, STD>(e, P, genv, c0, c1 SALP_STAMP_PASS);
    }
    else {
      SALP_STAMP(0);
      o = step_env<FMAX, FORCED, STD>(e, P, genv, c0, c1 SALP_STAMP_PASS);
    }
    const bool done = o.terminated || o.truncated;
    double rmax = o.rmax;
    bool have_rel = o.rel_valid;

    // ---- the per-step outputs
    // PACKED: the record's last float4, taken here (the values of the step's own episode, before the autoreset below)
    if constexpr (T::PACKED) {
      const uint32_t fl = (o.terminated ? 1u : 0u) | (o.truncated ? 0x100u : 0u) | (o.collision ? 0x10000u : 0u);
      const float4 last = make_float4(o.reward, __uint_as_float(fl), __uint_as_float((uint32_t)e.fc), __uint_as_float((uint32_t)e.ssf));
      if constexpr (T::TAILREG) reinterpret_cast<float4*>(record_block(io))[(rowbase + env) * RW4 + Q] = last;
      else *rec_stash = last;
    }
    if (!T::PACKED && !T::SUMMARY && active) {
      // reward: one dword per lane (256 B per wavefront); flags: one byte per lane.  (Rebuilding the
      // 64 flag bytes from a ballot and storing 16 dwords was measured: no faster in the memory
      // pipeline and slower overall, profiles/r01/ab_notes.md.)
      // (cache-policy bits on these small stores, and issuing them after the rows: measured, slower — r02 sessions 11, 14, 15)
      if (T::FULL || io.reward) io.reward[rowbase + env] = o.reward;
      if (T::FULL || io.terminated) io.terminated[rowbase + env] = o.terminated ? 1 : 0;
      if (T::FULL || io.truncated) io.truncated[rowbase + env] = o.truncated ? 1 : 0;
      if (T::EXTRAS && io.info) {
        int32_t* ip = io.info + (rowbase + env) * SALP_INFO_COLS;
        ip[SALP_INFO_FOOD_COLLECTED] = e.fc;
        ip[SALP_INFO_STEPS_SINCE_FOOD] = e.ssf;
        ip[SALP_INFO_COLLISION] = o.collision ? 1 : 0;
      }
    }
    // ---- the statistics and the record
    st_reward += (double)o.reward;
    if constexpr (T::NAV) {
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
    if constexpr (T::SUMMARY) {    // the float32 reward a rollout would have stored, added in step order in fp64; nothing below changes these
      const double r64 = (double)o.reward;
      const int end_now = o.terminated ? 1 : (o.truncated ? 2 : 0);     // terminated wins, as in the statistics below
      if constexpr (T::EVLDS) {
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

    // ---- the rare region: the wave statistics flush, the terminal observation, reset + placement, the foods selected again
    SALP_STAMP(6);
    // rare events: respawn of a collected food (snake:179-180), then same-step autoreset
    int todo = (o.collected && P.respawn) ? 1 : 0;
    const int F_base = P.F_base;
    if (SALP_RARE_TAKEN(o.collected || done)) {
      const DevParams& C = cold->P;   // rare path: constants from memory, not from scalar registers
      int limit = 50;
      if (o.collected || done) order_cache = -1;      // the food set (or the episode) changes
      if (io.stats) {
        if (lane < 16) wave_stats[lane] = 0ull;
        wave_sync();
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
        wave_sync();
        if (lane <= ST_EPRET) {
          const unsigned long long v = wave_stats[lane];
          if (v != 0) atomicAdd(&stats_replica->v[lane], v);
        }
        wave_sync();     // the placement's scratch and the tile rows come next
      }
      SALP_STAMP(10);
#pragma unroll 1
      for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && done && C.autoreset) {
          if (T::EXTRAS && io.final_obs && active) {
            float fo[T::OBS];
            if constexpr (T::LDSF) {   // the terminal observation sees the respawned food (pass 0)
              bool c_; int h_;
              scan_foods<KMAX, false, true>(food, C.F, e.x, e.y, 0.0, fq, c_, h_, nlive);
              if (__any(fq.tie)) exact_order_lds<KMAX>(food, C.F, K, e.x, e.y, fq);
              resolve<KMAX>(food, K, e.x, e.y, fq);
              observe_selected<KMAX, STD>(e, C, rmax, K, fq, nlive, false, 0.f, fo);
            } else if constexpr (T::REGF) {
              select_foods_reg<FMAX, KMAX, false, true>(e, ff, mir, K, (STD ? StdConsts::tie_c0 : C.tie_c0), fq, nlive);
              observe_selected<KMAX, STD>(e, C, rmax, K, fq, nlive, false, 0.f, fo);
            } else {
              observe<FMAX, KMAX, STD>(e, C, rmax, have_rel, o.rel, fo);
            }
            float4* dst = T::PACKED ? reinterpret_cast<float4*>(record_block(io)) + (rowbase + env) * RW4 + NQ     // the record's own tail
                                 : reinterpret_cast<float4*>(io.final_obs + (rowbase + env) * OD);
#pragma unroll
            for (int q = 0; q < T::QMAX; ++q)
              if (q < Q) dst[q] = make_float4(fo[4 * q], fo[4 * q + 1], fo[4 * q + 2], fo[4 * q + 3]);
          }
          if constexpr (T::LDSF) {
            todo = reset_core<STD>(e, C, genv, F_base);
            for (int k = 0; k < C.F; ++k) food.clear(k);
          } else {
            todo = reset_pose<FMAX, STD>(e, C, genv, F_base);
            if constexpr (T::REGF) {
#pragma unroll
              for (int k = 0; k < FMAX; ++k) { ff.clear(k, true); mir.clear(k); }
            }
          }
          limit = 100;
          rmax = STD ? StdConsts::R : C.R;
          have_rel = false;
        }
        if constexpr (T::LDSF) {
          wave_sync();
          place_food_coop<FMAX, STD>(e, food_lds + wave * FMAX * kWave, lane, C, genv, todo, limit);
          wave_sync();
        }
        else if constexpr (T::REGF) place_food_coop_reg<FMAX, STD, T::FOODREGS>(e, ff, mir, lane, C, genv, todo, limit, reinterpret_cast<double2*>(tile));
        else place_food<FMAX, STD>(e, C, genv, todo, limit);
        todo = 0;
      }
      SALP_STAMP(11);
      if constexpr (T::LDSF) {   // the food set (or the pose) changed: select again for the observation
        bool c_; int h_;
        scan_foods<KMAX, false, true>(food, C.F, e.x, e.y, 0.0, fq, c_, h_, nlive);
        if (__any(fq.tie)) exact_order_lds<KMAX>(food, C.F, K, e.x, e.y, fq);
        resolve<KMAX>(food, K, e.x, e.y, fq);
        have_rel = false;
      }
      if constexpr (T::REGF) {   // likewise (the exact order's scratch and the placement's are the same idle tile bytes, used in turn)
        select_foods_reg<FMAX, KMAX, false, true>(e, ff, mir, K, (STD ? StdConsts::tie_c0 : C.tie_c0), fq, nlive);
        have_rel = false;
      }
    }
    SALP_STAMP(7);

    // ---- the observation, its flush, the next action
    if (T::SUMMARY ? (t + 1 < Hrun) : (T::FULL || io.obs)) {     // SUMMARY: the row exists for the next action only
      float ob[T::OBS];
      if constexpr (T::REGF) {
        // all FMAX slots of every lane alive (the steady state with respawn) => every lane shows K foods
        if ((KMAX <= FMAX) && K >= 1 && __all(nlive == FMAX)) observe_selected<KMAX, STD, true>(e, P, rmax, K, fq, nlive, have_rel, o.rel, ob);
        else observe_selected<KMAX, STD>(e, P, rmax, K, fq, nlive, have_rel, o.rel, ob);
      } else if constexpr (T::LDSF) observe_selected<KMAX, STD>(e, P, rmax, K, fq, nlive, have_rel, o.rel, ob);
      else observe<FMAX, KMAX, STD>(e, P, rmax, have_rel, o.rel, ob);
      SALP_STAMP(8);
      // (per-lane 96-B rows stored straight from registers, without the LDS transpose: 2.1x slower, r01 ab_notes)
      [[maybe_unused]] v4f* gout = nullptr;
      if constexpr (!T::SUMMARY) gout = reinterpret_cast<v4f*>(io.obs + (rowbase + env0) * OD) + lane;
      if constexpr (T::SUMMARY) {
        // nothing is stored
      } else if constexpr (T::PACKED) {
        // the record rows through the tile, in one pass or (HALF) two of 32 rows; each pass is PJ 16-B-per-lane stores
        v4f* const rec0 = reinterpret_cast<v4f*>(record_block(io)) + (rowbase + env0) * RW4;
        const v4f* const tile4 = reinterpret_cast<const v4f*>(tile);
        const int skip4 = RW4 - TQ;                 // float4 the flush skips behind every tile row (wave-uniform)
#pragma unroll
        for (int i = 0; i < (T::PJ + 3) / 4; ++i) asm volatile("" : "+v"(rec_rows[i]));     // unpacked here, at every flush (see the plan)
        auto row_of = [&](int j) { return (int)((rec_rows[j >> 2] >> (8 * (j & 3))) & 0xFFu); };
        // whole store instructions of an unpredicated K = 3 launch carry no test at all
        auto moves = [&](int j) { return (!RAGGED && KMAX == 3 && (j + 1) * kWave <= T::TILE_ROWS * T::QPMAX) ? true : row_of(j) != 0xFF; };
        float4 tail = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (!T::TAILREG) {
          // every lane's, before ANY lane writes a row over the stash: the rows of other lanes cover it, which the compiler,
          // reasoning about one lane, cannot see — without the barrier it sank this read below the row writes
          tail = *rec_stash;
          wave_sync();
        }
#pragma unroll
        for (int h = 0; h < (T::HALF ? 2 : 1); ++h) {
          if (!T::HALF || (lane >> 5) == h) {
#pragma unroll
            for (int q = 0; q < T::QMAX; ++q)
              if (q < Q) ((q & 1) ? myrow_odd : myrow_even)[q] = make_float4(ob[4 * q], ob[4 * q + 1], ob[4 * q + 2], ob[4 * q + 3]);
            if constexpr (!T::TAILREG) myrow4[Q] = tail;
          }
          wave_sync();
          v4f tv[T::PJ];
#pragma unroll
          for (int j = 0; j < T::PJ; ++j)
            if (moves(j)) {
              if constexpr (T::TAILREG) tv[j] = *flush_src[j];        // the swizzled six-column tile of the unpacked signatures
              else tv[j] = tile4[j * kWave + lane + row_of(j) * (T::PITCH / 4 - TQ)];
            }
          v4f* const pass0 = rec0 + h * T::TILE_ROWS * RW4;
#pragma unroll
          for (int j = 0; j < T::PJ; ++j)
            if (moves(j)) __builtin_nontemporal_store(tv[j], &pass0[j * kWave + lane + row_of(j) * skip4]);
          wave_sync();     // this pass's reads before the next writes of the tile
        }
      } else if constexpr (T::HALF) {
        // float4 f = j*64 + lane (j = 0..2) of a half lives at tile row f / 6, column f % 6 (flush_src[0..2]) and goes to global
        // float4 (3 h + j) * 64 + lane of the wavefront's 64-row block: the same 1-KB stores as the full plan, three per half
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if ((lane >> 5) == h) {
#pragma unroll
            for (int q = 0; q < T::QMAX; ++q)
              ((q & 1) ? myrow_odd : myrow_even)[q] = make_float4(ob[4 * q], ob[4 * q + 1], ob[4 * q + 2], ob[4 * q + 3]);
          }
          wave_sync();
          v4f tv[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) tv[j] = *flush_src[j];
#pragma unroll
          for (int j = 0; j < 3; ++j) __builtin_nontemporal_store(tv[j], &gout[(3 * h + j) * kWave]);
          wave_sync();     // the reads of this half before the writes of the next
        }
      } else {
#pragma unroll
      for (int q = 0; q < T::QMAX; ++q)   // 16-B LDS stores, conflict-free (see the tile layout above)
        if (q < Q) ((q & 1) ? myrow_odd : myrow_even)[q] = make_float4(ob[4 * q], ob[4 * q + 1], ob[4 * q + 2], ob[4 * q + 3]);
      wave_sync();
      {
        v4f tv[T::QMAX];
#pragma unroll
        for (int j = 0; j < T::QMAX; ++j)
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
        if constexpr (!RAGGED && T::QMAX == 6 && !T::MULTI) {   // the write-bound one-food kernel; the VALU-bound multi-food ones: +1 %, not used
          v4f* const gout4 = gout + 4 * kWave;     // the instruction's immediate offset reaches 4095 B: two bases
#pragma unroll
          for (int j = 0; j < T::QMAX - 1; ++j)
            asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1 nt"
                         :: "v"(j < 4 ? gout : gout4), "v"(tv[j]), "n"((j & 3) * kWave * 16) : "memory");
          asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1 nt\n\ts_nop 0"
                       :: "v"(gout4), "v"(tv[T::QMAX - 1]), "n"(((T::QMAX - 1) & 3) * kWave * 16) : "memory");
        } else
#pragma unroll
        for (int j = 0; j < T::QMAX; ++j)
          if (j < Q && (!RAGGED || lds_off[j] >= 0)) __builtin_nontemporal_store(tv[j], &gout[j * kWave]);
      }
      wave_sync();
      }
      // the next step's action from this step's row, while the row stores are in flight (the last step needs none)
      if constexpr (T::POLICY) {
        if (T::SUMMARY || t + 1 < Hrun) {
          float av[AD];
          if constexpr (T::SAMPLED) {
            const U4 nw = philox4x32_10((uint32_t)genv, (uint32_t)(genv >> 32), noise0 + (uint32_t)(t + 1), 3u, P.seed[0], P.seed[1]);
            float zv[AD];
            zv[0] = policy_normal(nw.x, nw.y);
            if constexpr (!FORCED) zv[1] = policy_normal(nw.z, nw.w);
            if constexpr (T::WIDE) policy_eval_wide<AD, true>(io.act, pol_off, ob, zv, av, lp);
            else
            policy_eval_sampled<T::OBS, AD>(io.act, pol_off, ob, zv, av, lp);
          } else if constexpr (T::WIDE) {
            const float zv[AD] = {};
            float unused = 0.f;
            policy_eval_wide<AD, false>(io.act, pol_off, ob, zv, av, unused);
          } else
          policy_eval<T::OBS, AD>(io.act, pol_off, ob, av);
          take_actions(av, a0, a1);
        }
      }
    }
    // One-food kernel (write-bound): drain this step's stores before the next step.  Measured
    // (profiles/r01/ab_notes.md): letting stores run ahead (vmcnt(9)) is 2-6 % SLOWER than draining —
    // wavefronts that stay in step keep the write stream of all CUs inside one contiguous [N x 96 B] slab
    // at a time.  The multi-food kernels are issue-bound at 2 wavefronts per SIMD: there the drain is a
    // stall nothing hides (-6.4 % without it, profiles/r02/ab_notes.md session 2).
    if constexpr (!T::MULTI && !T::SUMMARY) __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)   (SUMMARY: the loop has no store to drain)
    SALP_STAMP(9);
  }
  SALP_STAMPS_CLOSE(lane == 0 && rows > 0, (env0 - env_begin) / kWave);

  // ---- store the state and the record
  if (rows > 0 && active) {
    const DevParams& C = cold->P;
    const DevState CS = cold->S;
    if constexpr (T::LDSF) {
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
    if constexpr (T::NAV) {         // the env's record: five 16-byte stores (a lane that took no step writes back what it read)
      int4* const rp = reinterpret_cast<int4*>(record_block(io)) + env * (SALP_NAV_WORDS / 4);
      rp[0] = make_int4(nv_steps, nv_status, __double2loint(nv_path), __double2hiint(nv_path));
      rp[1] = make_int4(__double2loint(nv_lat), __double2hiint(nv_lat), __double2loint(nv_xmin), __double2hiint(nv_xmin));
      rp[2] = make_int4(__double2loint(nv_xmax), __double2hiint(nv_xmax), __double2loint(nv_ymin), __double2hiint(nv_ymin));
      rp[3] = make_int4(__double2loint(nv_ymax), __double2hiint(nv_ymax), __double2loint(e.x), __double2hiint(e.x));
      rp[4] = make_int4(__double2loint(e.y), __double2hiint(e.y), 0, 0);
    } else
    if constexpr (T::SUMMARY) {     // the env's record: two 16-byte stores
      int4* const rp = reinterpret_cast<int4*>(record_block(io)) + env * 2;
      if constexpr (T::EVLDS) {
        rp[0] = ev_lds[0];
        rp[1] = ev_lds[kWave];
      } else {
        rp[0] = make_int4(__double2loint(ev_ret), __double2hiint(ev_ret), __double2loint(ev_first_ret), __double2hiint(ev_first_ret));
        rp[1] = make_int4(ev_first_len, ev_first_end, ev_episodes, ev_food);
      }
    }
  }

  // ---- the launch statistics
  if (io.stats) {
    // reward sum and env-step count: wavefront shuffles, the four wavefronts' sums through 64 bytes of the (now idle)
    // first tile, then two 64-bit integer global atomics per WORKGROUP (per wavefront they cost the H = 1 step kernel 8 %:
    // 8192 atomics on a 14-us launch, profiles/r03/ab_notes.md session 10)
    if (!active || rows == 0) st_reward = 0.0;
    const double wr = wave_sum(st_reward);
    // NAV: the steps the lanes actually took (a stopped env takes none)
    const int wact = wave_sum((active && rows > 0) ? (T::NAV ? nv_steps - nv_steps0 : 1) : 0);
    unsigned long long* const blk = reinterpret_cast<unsigned long long*>(lds);
    __syncthreads();                               // every wavefront is past its last tile flush
    if (lane == 0) {
      blk[2 * wave] = (unsigned long long)__double2ll_rn(wr * SALP_FIXED_SCALE);
      blk[2 * wave + 1] = (unsigned long long)((long long)wact * (T::NAV ? 1 : H));
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
  if constexpr (ACT == ACT_POLICY || ACT == ACT_POLICY_SAMPLED || ACT == ACT_POLICY_WIDE || ACT == ACT_POLICY_WIDE_SAMPLED) {
    if (sig == kSigNav) {
      if constexpr ((ACT == ACT_POLICY || ACT == ACT_POLICY_WIDE) && FMAX == 1 && KMAX == 3 && FORCED) return picked<FMAX, KMAX, FORCED, STD, kSigNav, RAGGED, ACT>();
      else return RolloutPick{nullptr, -1};
    }
    if (sig == kSigSummary) return picked<FMAX, KMAX, FORCED, STD, kSigSummary, RAGGED, ACT>();
    if (sig == kSigPacked) return picked<FMAX, KMAX, FORCED, STD, kSigPacked, RAGGED, ACT>();
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
  if (act == ACT_POLICY_WIDE || act == ACT_POLICY_WIDE_SAMPLED) {     // the wide evaluation (salp_policy_wide.h): one food, K = 3, the same signatures
    if constexpr (FMAX == 1 && KMAX == 3) {
      if ((sig == kSigMain || sig == kSigSummary || sig == kSigPacked) && act == ACT_POLICY_WIDE_SAMPLED)
        return forced ? pick_sig<FMAX, KMAX, true, STD, RAGGED, ACT_POLICY_WIDE_SAMPLED>(sig) : pick_sig<FMAX, KMAX, false, STD, RAGGED, ACT_POLICY_WIDE_SAMPLED>(sig);
      if ((sig == kSigMain || sig == kSigSummary || sig == kSigNav || sig == kSigPacked) && act == ACT_POLICY_WIDE)
        return forced ? pick_sig<FMAX, KMAX, true, STD, RAGGED, ACT_POLICY_WIDE>(sig) : pick_sig<FMAX, KMAX, false, STD, RAGGED, ACT_POLICY_WIDE>(sig);
    }
    return RolloutPick{nullptr, -1};
  }
  if ((sig == kSigMain || sig == kSigSummary || sig == kSigPacked) && act == ACT_POLICY_SAMPLED)   // the same signatures but the navigation, sampling
    return forced ? pick_sig<FMAX, KMAX, true, STD, RAGGED, ACT_POLICY_SAMPLED>(sig) : pick_sig<FMAX, KMAX, false, STD, RAGGED, ACT_POLICY_SAMPLED>(sig);
  if ((sig == kSigMain || sig == kSigSummary || sig == kSigNav || sig == kSigPacked) && act == ACT_POLICY)   // the in-kernel policy exists for the main-only output signature, the packed record, the summary and the navigation record
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
