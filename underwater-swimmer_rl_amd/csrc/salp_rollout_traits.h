// salp_rollout_traits.h — what the rollout kernel (salp_rollout_kernel.h) is a function of: the launch arguments IOPtrs and
// ColdBlock with the named meanings of their overloaded slots, and RolloutTraits, every compile-time switch and size of one
// instantiation in one place (its launch bound and its LDS bytes per workgroup among them, the latter pinned below to the
// table of DESIGN.md §3.1).  Host and device code both read this file; it holds no device function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/salp_vec.h"
#include "salp_device.h"
#include "salp_food_reg.h"

using namespace salp;

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int kBlock = 256;
constexpr int kWave = 64;

// Where the actions of a launch come from (template parameter ACT).
// ACT_GEN = actions are generated in the kernel (salp_vec_rollout with act == NULL): no read stream at
// all — the per-step 256-B action read costs the write stream ~10 % (HBM read/write turnarounds,
// profiles/r01/ab_notes.md) — and, if act_out is given, the actions are written out instead.
// ACT = ACT_POLICY: the actions are a function of the observations (salp_vec_rollout_policy): the action of step 0 is the
// policy (salp_policy.h) applied to the env's current observation, computed in the prologue with the step's own
// functions; the action of step t + 1 is the policy applied to the row just written to obs[t], evaluated from the
// registers behind the tile flush, while the row stores drain.  No read stream; act_out as with ACT_GEN.
// ACT = ACT_POLICY_SAMPLED: the same closed loop with the stochastic form of a Gaussian policy (salp_vec_rollout_policy_sampled,
// salp_vec_evaluate_policy_sampled): the action of step t is sampled with the policy's noise block n0 + t of the env, n0 =
// the policy's noise step read from its device block at entry; its log-probability goes to logp_out with the action.
// ACT = ACT_POLICY_WIDE / ACT_POLICY_WIDE_SAMPLED: the same two closed loops with the policy evaluated on the matrix cores
// (salp_policy_wide.h: hidden widths up to 256); one-food kernels only, one wavefront per SIMD.
enum { ACT_READ = 0, ACT_GEN = 1, ACT_POLICY = 2, ACT_POLICY_SAMPLED = 3, ACT_POLICY_WIDE = 4, ACT_POLICY_WIDE_SAMPLED = 5 };

// Output signatures (template parameter SIG): kSigMain = obs, reward, terminated, truncated and nothing else — every
// store of the step loop is unconditional, so the compiler can count the stores issued after the action prefetch and wait
// for the prefetch alone; kSigExtras = the same four plus final_obs and / or info (salp_vec_step, rollouts that keep the
// terminal observations): the four main streams stay unconditional, only the extras are tested (the terminal rows are
// written in the rare-event region, the three info words per step); kSigPartial = some main output is NULL: every
// store is tested, the step ends in a full drain (a 12-food rollout with final_obs ran 22 % slower in that form,
// profiles/r03/ab_notes.md session 15).  The one-wavefront predicated launches exist as kSigMain and kSigPartial only.
// kSigPacked = ONE stream of transition records (salp_vec_step_packed / salp_vec_rollout_packed): no per-lane reward / flag /
// info stores at all; unpredicated and predicated, K = 3 and generic K; no in-kernel action generation.  K = 3 also with the
// in-kernel policy, deterministic and sampling (salp_vec_rollout_policy_packed, include/salp_vec_policy_packed.h).
// kSigSummary = NO per-step output: one record of SALP_EVAL_WORDS words per env at the end of the launch
// (salp_vec_evaluate_policy); exists for the in-kernel policy and K = 3 only, unpredicated and predicated.
// kSigNav = the summary kernel's loop with a per-env stop at a goal and one navigation record of SALP_NAV_WORDS words per env
// (salp_vec_evaluate_navigation); exists for one food, K = 3, forced breathing and the deterministic in-kernel policy only —
// four kernels, in the two one-food units.  Asked of anything else the choice is empty (fn NULL): the host refuses first.
enum { kSigPartial = 0, kSigMain = 1, kSigExtras = 2, kSigPacked = 3, kSigSummary = 4, kSigNav = 5 };

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
    float* logp_out;      // ACT_POLICY_SAMPLED (whose signatures have no info stream — the packed record carries the counters): [H][n] or null
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
// The second meanings of three slots, written down once and used by both sides (the kernel reads, salp_vec.hip sets):
//   record_block: io.obs of kSigPacked ([H][n] transition records), kSigSummary ([n][SALP_EVAL_WORDS] words) and kSigNav
//                 ([n][SALP_NAV_WORDS] words) — one block of records instead of the observation stream;
//   accumulate:   io.final_obs != NULL of kSigSummary and kSigNav — the records are read first and continued
//                 (SALP_EVAL_ACCUMULATE); the pointer's value is never used;
//   packed_has_final: io.final_obs != NULL of kSigPacked — the records carry a terminal-observation tail, written in
//                 place (behind the record's own float4s, not through the pointer);
//   set_policy_block: io.act of ACT_POLICY / ACT_POLICY_SAMPLED — the policy's device block (salp_policy.h).  It has no
//                 reader of its own: read through a function, the pointer moved the instruction order of eight one-food policy
//                 kernels (profiles/r10/refactor_notes.md); the kernel reads io.act.
__host__ __device__ __forceinline__ float* record_block(const IOPtrs& io) { return io.obs; }
__host__ __device__ __forceinline__ bool accumulate(const IOPtrs& io) { return io.final_obs != nullptr; }
__host__ __device__ __forceinline__ bool packed_has_final(const IOPtrs& io) { return io.final_obs != nullptr; }
inline void set_record_block(IOPtrs& io, float* records, bool flag) { io.obs = records; io.final_obs = flag ? records : nullptr; }
inline void set_policy_block(IOPtrs& io, const float* block) { io.act = block; }

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

// Every compile-time switch and size of salp_rollout_kernel<FMAX, KMAX, FORCED, STD, SIG, RAGGED, ACT>.
// RAGGED = false: every wavefront of the launch is either full (64 envs) or empty, so no store is
// predicated and the compiler can count the stores issued after the action prefetch (it then waits
// for the prefetch alone instead of draining all stores with s_waitcnt vmcnt(0) every step).
// RAGGED = true: the same loop with per-lane predicates; the host launches it for the last
// n % 64 envs only (one wavefront).  `env_begin/env_end`: the env range of this launch.
// STD = false: where the hot path's constants come from (open_consts, salp_params.h) — the device copy, function by
// function, for the 4- and 8-slot kernels; the by-value launch parameters for the others (MEMC).
template <int FMAX_, int KMAX_, bool FORCED_, bool STD_, int SIG_, bool RAGGED_, int ACT_>
struct RolloutTraits {
  static constexpr int FMAX = FMAX_, KMAX = KMAX_, SIG = SIG_, ACT = ACT_;
  static constexpr bool FORCED = FORCED_, STD = STD_, RAGGED = RAGGED_;
  static constexpr bool GEN = ACT == ACT_GEN;
  static constexpr bool WIDE = ACT == ACT_POLICY_WIDE || ACT == ACT_POLICY_WIDE_SAMPLED;     // the evaluation of salp_policy_wide.h
  static constexpr bool SAMPLED = ACT == ACT_POLICY_SAMPLED || ACT == ACT_POLICY_WIDE_SAMPLED;
  static constexpr bool POLICY = ACT == ACT_POLICY || SAMPLED || WIDE;
  static_assert(!WIDE || (FMAX_ == 1 && KMAX_ == 3), "the wide policy evaluation exists in the one-food kernels only");
  // SIG 4 (kSigSummary): NO per-step output at all — salp_vec_evaluate_policy.  record_block(io) is the block of per-env summary
  // records ([n][SALP_EVAL_WORDS] words, include/salp_vec.h), accumulate(io) says that the records are read first and continued
  // (SALP_EVAL_ACCUMULATE).  The observation is formed in registers for the policy alone: no tile write, no flush, no
  // reward / flag / action store; the record leaves next to the state write-back.  The LDS layout is that of the twin policy
  // kernel (the rare paths still borrow the tile's bytes, the mirror sits behind it): LDS limits none of these kernels.
  // SIG 5 (kSigNav): the summary kernel's loop with a per-env `running` predicate and a navigation record — salp_vec_evaluate_navigation.
  // record_block(io) is the block of records ([n][SALP_NAV_WORDS] words), accumulate(io) = SALP_EVAL_ACCUMULATE, io.nav_line the
  // trials' start / goal, io.nav_radius the goal radius, io.nav_track the optional positions.  A lane that is not running is not
  // stepped: nothing of its state, statistics or record moves; a wavefront with no running lane leaves the step loop.
  static constexpr bool NAV = SIG == kSigNav;
  static constexpr bool SUMMARY = SIG == kSigSummary || NAV;     // everything the two share: no per-step output, no tile write
  static_assert(!POLICY || ((SIG == 1 || SIG == 3 || SIG == 4 || SIG == 5) && KMAX == 3), "policy kernels: the main-only, the packed, the summary and the navigation signature, K = 3");
  static_assert(!SUMMARY || POLICY, "the summary signature exists for the in-kernel policy only");
  static_assert(!NAV || (FMAX == 1 && FORCED && (ACT == ACT_POLICY || ACT == ACT_POLICY_WIDE)), "the navigation signature: one food, forced breathing, the deterministic policy");
  // (the summary kernels the other way round — by value with 4 / 8 slots, the device copy with 16: with no store in the step loop
  // the twins' choice left 300-560 scalar registers spilled and 68-196 B of scratch reserved in four of them; so chosen, none
  // of the 40 holds scratch where its twin holds none, profiles/r06/eval_kernel_resources.txt)
  static constexpr bool MEMC = !STD && KMAX == 3 && (SIG == 4 ? FMAX == 16 : (FMAX == 4 || FMAX == 8));
  // FULL = the common rollout signature (act, obs, reward, terminated, truncated all present; no
  // final_obs / info): no per-step null tests.
  static constexpr bool FULL = SIG != 0;         // obs, reward, terminated, truncated all present: their stores are unconditional
  static constexpr bool EXTRAS = SIG != 1 && !SUMMARY;   // final_obs / info may be present (tested per use; SIG 0: every output is tested)
  // SIG 3 (kSigPacked): ONE output stream of transition records (include/salp_vec.h "Packed transition record") — the
  // observation row plus one float4 (reward, flags word, food_collected, steps_since_food) — through the tile; record_block(io)
  // is the record block, packed_has_final(io) says that the rows carry a terminal-observation tail
  static constexpr bool PACKED = SIG == kSigPacked;
  // TAILREG: the unpredicated 8-slot packed kernel stores that last float4 straight from registers (one 16-B store per
  // lane where the other signatures issue their reward / flag / info stores) and keeps the tile of the unpacked
  // signatures: 40960 B of LDS per workgroup is exactly four workgroups per CU, a seven-column tile (45056 B) is three.
  // Not with the in-kernel policy: its 8-slot kernels run one wavefront per SIMD (waves_per_simd below), one workgroup per CU,
  // so LDS limits nothing there; they take the seven-column tile and the stash like every other slot count, and every store
  // of the record stays a whole-line store.
  static constexpr bool TAILREG = PACKED && !RAGGED && KMAX == 3 && FMAX == 8 && !POLICY;
  static constexpr int OBS = 12 + 4 * KMAX;        // floats of the widest observation row
  static constexpr int AD = FORCED ? 1 : 2;        // action components
  static constexpr int QMAX = 3 + KMAX;          // float4 per observation row
  static constexpr int QPMAX = QMAX + ((PACKED && !TAILREG) ? 1 : 0);   // float4 columns of a tile row
  // LDS tile of the wavefront's 64 observation rows.  Banking (MI355X_MICROARCH.md §LDS): ds_write_b128 goes
  // in 8 groups of 8 lanes over banks (a/4) mod 32, ds_read_b128 in 4 groups of 16 lanes ({0-3,12-15,20-27},
  // ...) over banks (a/4) mod 64.  K = 3 (Q = 6 float4 per row): unpadded 96-B rows with the float4 column
  // XOR-ed by bit 2 of the row — conflict-free for the row writes AND for the flush reads (profiles/isa_lds_model.py;
  // the 112-B padded pitch of round 1 was conflict-free for the writes only: 2-way on the reads).
  // Other K (generic instantiation, Q possibly odd): the padded pitch.
  // PACKED: unpadded rows of Q + 1 float4 with no swizzle.  K = 3: 7 float4 = 112 B, an ODD number of float4, so eight
  // consecutive rows start in eight different 16-B bank groups (writes conflict-free) and the flush reads float4 j*64 + lane
  // of a linear tile (reads conflict-free): profiles/isa_lds_model.py PACKED.  Generic K: rows of QPMAX float4, not modelled.
  static constexpr bool SWZ = (KMAX == 3) && (!PACKED || TAILREG);
  static constexpr int PITCH = (PACKED && !TAILREG) ? 4 * QPMAX : (SWZ ? 4 * QMAX : 4 * QMAX + 4);     // LDS row pitch in floats
  // Where the food positions of a multi-food env live: up to 12 slots in VGPRs with an fp32 mirror in LDS
  // (salp_food_reg.h), above that in LDS (salp_food_lds.h); one food is plain registers.
  static constexpr bool REGF = FMAX > 1 && (FMAX <= 12 || KMAX == 3);   // K = 3: every slot count; generic K: up to 12 slots
  static constexpr bool LDSF = FMAX > 1 && !REGF;                         // generic K with 13..16 slots
  static constexpr bool MULTI = REGF || LDSF;
  // Per-wavefront LDS region: the observation tile (64 rows of PITCH floats) and, for the register-food kernels, the
  // fp32 mirror of the food positions behind it (8 B per slot and lane, salp_food_reg.h; lives for the whole launch).
  // 12 slots, K = 3: 6144 + 6144 B per wavefront, 49 KB per workgroup -> 3 workgroups per CU.  The tile's bytes, idle in
  // the middle of a step, are lent to the rare paths as scratch: the exact order's distances (8 B per slot and lane,
  // <= the tile for every instantiation) and the placement's accepted points.
  // HALF: a tile of 32 rows, written and flushed twice per step (lanes 0-31, then 32-63): 3072 instead of 6144 B per wavefront.
  // The 16-slot kernel's mirror is 8192 B per wavefront: 57344 B per workgroup allowed two workgroups per CU, 45056 B allow three
  // (and without the fp32 register copies it holds 159 VGPRs <= 168).
  static constexpr bool HALF = !RAGGED && REGF && KMAX == 3 && FMAX == 16 && STD;
  static constexpr int TILE_ROWS = HALF ? kWave / 2 : kWave;
  static constexpr int TILE_FLOATS = TILE_ROWS * PITCH;
  // SUMMARY, register-food kernels: the env's record (32 B per lane) is kept in LDS behind the mirror and updated there every
  // step — these kernels sit at their register limits (eight more registers across the loop put 12-132 B of scratch into the
  // 4-slot ones, profiles/r06/ab_notes.md) and LDS limits none of them; the one-food kernels keep it in registers.
  static constexpr bool EVLDS = SUMMARY && FMAX > 1;
  static constexpr int EV_FLOATS = EVLDS ? kWave * SALP_EVAL_WORDS : 0;
  static constexpr int WAVE_FLOATS = TILE_FLOATS + (REGF ? kWave * 2 * FMAX : 0) + EV_FLOATS;
  static_assert(!REGF || (4 * FMAX <= TILE_ROWS * PITCH && 96 <= TILE_ROWS * PITCH), "the placement's FMAX accepted points (16 B each) must fit in the tile");
  // PACKED: 16-B-per-lane stores of one tile pass (the flush plan, Tile in salp_rollout_parts.h)
  static constexpr int PJ = PACKED ? (TILE_ROWS * QPMAX + kWave - 1) / kWave : 1;
  // REGF: whether the fp32 roundings of the food positions are kept in registers next to the LDS mirror (salp_food_reg.h)
  static constexpr bool FOODREGS = food_in_registers(FMAX, KMAX, STD, SIG == 1 || SIG == 4) && !HALF;
  // LDS of the generic <16, 8> kernel's food block (salp_food_lds.h: 16 B per slot and lane), which exists nowhere else
  static constexpr int FOOD_LDS_BYTES = LDSF ? (kBlock / kWave) * FMAX * kWave * (int)sizeof(double2) : 0;
  // LDS bytes per workgroup: per wavefront the tile, the mirror and the summary record; and the LDS-food block
  static constexpr int LDS_BYTES = (kBlock / kWave) * WAVE_FLOATS * (int)sizeof(float) + FOOD_LDS_BYTES;

  // Wavefronts per SIMD the launch bounds ask for (workgroups of 256 threads per CU), by food-slot count:
  //   one food 4;  4 / 8 slots 4 — 128 VGPRs, their LDS (32 / 40 KB) allows four workgroups per CU; without the bound several
  //   signatures landed on 129 = three per SIMD, up to 22 % slower (profiles/r03/ab_notes.md sessions 14, 20);  12 slots 3 —
  //   <= 168 VGPRs, 49 KB of LDS (four: a timing build at 128 VGPRs / 36 KB was 13 % slower, session 17);  16 slots 3 for the
  //   literal-constant unpredicated kernels (half-height tile, session 19), else 2;  generic K: 2 (12 slots) / 1 (16 slots).
  //   The packed signature keeps every row (its 8-slot kernel keeps the six-column tile, TAILREG above); its one-wavefront
  //   predicated 8-slot twin has the seven-column tile, 45 KB: 3.
  //   The policy kernels (ACT_POLICY): the first hidden layer's activations are up to 64 VGPRs on top of the step's own.  One food
  //   and 4 slots: 2 (256 registers, no scratch).  8 slots and more, and every predicated launch: 1 — at 2 they spilled 50-580 B
  //   per lane to scratch inside the step loop; at 1 the wavefront owns the SIMD's 512 registers and what does not fit in the
  //   256 VGPRs is parked in AGPRs (v_accvgpr_write / _read), not in memory (profiles/r05/policy_kernel_resources.txt).
  static constexpr int waves_per_simd() {
    // The sampling policy kernels (ACT_POLICY_SAMPLED) take their deterministic twins' bounds, but for six unpredicated kernels
    // that at 2 held 2-16 scratch instructions (12-36 B per lane) where the twin holds fewer or none — the 4-slot rollout kernels,
    // the free-breathing 4-slot summary kernel with literal constants, the free-breathing one-food summary kernel with run-time
    // constants: 1.  From the code-object metadata of all 80: profiles/r07/sampled_kernel_resources.txt.
    // The packed policy kernels (sig 3, salp_vec_rollout_policy_packed) take the bounds of their main-only twins (sig 1), sampling
    // or not: the record's last float4 waits in LDS, not in registers (profiles/r16/policy_packed_kernel_resources.txt).
    // The wide policy kernels: 1 — the stored hidden layer of one env half is up to 128 registers on top of the step's own, the
    // accumulators of two tiles 32 more; the wavefront owns the SIMD's 512 registers (profiles/r05/policy_wide_kernel_resources.txt).
    if (WIDE) return 1;
    if (SAMPLED && !RAGGED && FMAX == 4 && (SIG == 1 || SIG == 3 || !FORCED)) return 1;
    // Two more packed kernels go to 1, by the same rule (scratch at 2 where the twin holds less): the unpredicated one-food
    // sampling kernel with run-time constants (12 B, its twin none) and the unpredicated free-breathing 4-slot kernel (20 B, its twin 12).
    if (SIG == 3 && SAMPLED && !RAGGED && FMAX == 1 && !STD) return 1;
    if (SIG == 3 && POLICY && !SAMPLED && !RAGGED && FMAX == 4 && !FORCED) return 1;
    if (SAMPLED && !RAGGED && FMAX == 1 && SIG == 4 && !STD && !FORCED) return 1;
    // The summary kernels (sig 4) take their twins' bounds, but for the unpredicated 4-slot kernel with run-time constants: 1 (at 2
    // it sat at 255-256 VGPRs with 12-132 B of scratch, its twin holds 0-12 B; at 1 258-272 registers, 2-16 of them AGPRs, none).
    // From the code-object metadata of all 40: profiles/r06/eval_kernel_resources.txt.
    if (POLICY && SIG == 4 && FMAX == 4 && !STD && !RAGGED) return 1;
    // The navigation kernels (sig 5, one food): 1 — the record and the trial's line are 26 more registers across the loop than the
    // summary kernel's 224; at 2 the unpredicated kernel with literal constants held 136 B of scratch (33 VGPRs spilled).
    if (POLICY && SIG == 5) return 1;
    if (POLICY) return (RAGGED || FMAX >= 8) ? 1 : 2;
    if (SIG == 3 && RAGGED && KMAX == 3 && FMAX == 8) return 3;
    return FMAX <= 1 ? 4 : (KMAX != 3 ? (FMAX <= 12 ? 2 : 1) : (FMAX <= 8 ? 4 : (FMAX <= 12 ? 3 : ((STD && !RAGGED) ? 3 : 2))));
  }
};

// LDS per workgroup, the table of DESIGN.md §3.1 (K = 3; literal or run-time constants alike but for 16 slots): what the
// occupancy tests see on the GPU only, held here at compile time.  {slots, predicated, literal constants} -> unpacked, packed.
template <int FMAX, bool STD, bool RAGGED, int SIG> constexpr int lds_bytes_k3 = RolloutTraits<FMAX, 3, true, STD, SIG, RAGGED, ACT_READ>::LDS_BYTES;
template <int FMAX, bool STD, bool RAGGED> constexpr bool lds_row_is(int unpacked, int packed) {
  return lds_bytes_k3<FMAX, STD, RAGGED, kSigPartial> == unpacked && lds_bytes_k3<FMAX, STD, RAGGED, kSigMain> == unpacked &&
         (RAGGED || lds_bytes_k3<FMAX, STD, false, kSigExtras> == unpacked) && lds_bytes_k3<FMAX, STD, RAGGED, kSigPacked> == packed;
}
static_assert(lds_row_is<1, true, false>(24576, 28672) && lds_row_is<1, false, true>(24576, 28672), "DESIGN.md §3.1: one food");
static_assert(lds_row_is<4, true, false>(32768, 36864) && lds_row_is<4, false, true>(32768, 36864), "DESIGN.md §3.1: 4 slots");
static_assert(lds_row_is<8, true, false>(40960, 40960) && lds_row_is<8, false, false>(40960, 40960), "DESIGN.md §3.1: 8 slots");
static_assert(lds_row_is<8, true, true>(40960, 45056) && lds_row_is<8, false, true>(40960, 45056), "DESIGN.md §3.1: 8 slots, predicated twin");
static_assert(lds_row_is<12, true, false>(49152, 53248) && lds_row_is<12, false, true>(49152, 53248), "DESIGN.md §3.1: 12 slots");
static_assert(lds_row_is<16, true, false>(45056, 47104), "DESIGN.md §3.1: 16 slots, literal constants, unpredicated");
static_assert(lds_row_is<16, true, true>(57344, 61440) && lds_row_is<16, false, false>(57344, 61440) && lds_row_is<16, false, true>(57344, 61440), "DESIGN.md §3.1: 16 slots, other constants");

}  // namespace
