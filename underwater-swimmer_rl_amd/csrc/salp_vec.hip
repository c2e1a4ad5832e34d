// salp_vec.hip — the C ABI of include/salp_vec.h: host code only.  The service kernels it launches (reset / observe,
// state snapshots, generated actions, reseed, policy relayout and noise step) are salp_service_kernels.h.  The fused
// step/rollout kernel is salp_rollout_kernel.h; its instantiations are compiled by the salp_rollout_*.hip units and
// reached through their rollout_unit_fn functions.  What is decided before a GPU is touched lives in host functions that
// are under test without one: the config's defaults and ranges, the launch parameters derived from it and the ranges of
// a snapshot (default_config, validate, make_params, is_std, check_snapshot: salp_params.h); a policy descriptor's ranges,
// the map from the public weight layout to the device block, the block's header and the allocations' sizes (salp_policy.h).
// The policy object behind a salp_policy_t, shared with salp_robot.hip, is salp_policy_object.h; the two functions through
// which the robot library reaches this unit's policy kernels are defined here (salp_policy_upload.h).
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/salp_vec_policy_packed.h"
#include "../../include/salp_vec_policy_wide.h"
#include "salp_host.h"
#include "salp_policy_object.h"
#include "salp_rollout_kernel.h"
#include "salp_service_kernels.h"

static_assert(POLICY_WAVE == kWave, "salp_policy.h states the wavefront rule with its own constant");

// ------------------------------------------------------------------ host side (fail, HIP_TRY, CallFrame, launch_1d, staged(): salp_host.h)
struct salp_vec {
  salp_config_t cfg;
  DevParams P;
  DevState S;
  int device;
  int64_t n;
  uint64_t seed;
  int64_t global_step;
  int obs_dim, act_dim, F, K;
  int fmax, kmax;
  int std_consts;        // constants equal the reference defaults -> literal-constant kernels
  DevStats* stats;       // device, SALP_STATS_REPLICAS replicas
  int stats_enabled;
  ColdBlock* cold;       // device copy of P and S for the rollout kernel's rare paths
  StageBuffer stage;     // staging for host-pointer calls (grown on demand)
  float* act_buf;        // device-generated actions when the caller gives no act_out
  size_t act_bytes;
  size_t nf_rows;
  hipStream_t last_stream;   // the stream of the handle's most recent launch: what get_stats / destroy wait for
  int64_t last_launch[8];    // salp_vec_last_launch
  int64_t last_sigs[2];      // salp_vec_last_launch_signatures
  const void* last_kernel;   // the main (else the predicated) kernel of the most recent launch: salp_vec_last_kernel_resources
  int last_wide;             // salp_vec_last_launch_policy_wide: the most recent launch ran the kernels of salp_policy_wide.h
};

struct salp_policy : PolicyObject {     // salp_policy_object.h; last_stream: create / update / noise-step writes, sampled calls included
  salp_vec* h;               // the handle it is bound to
};

namespace {

// make_params(), is_std() and the config's ranges: salp_params.h (host functions, under test without a GPU).
int validate(const salp_config_t* c) {
  const char* why = "";
  const int rc = salp::validate(c, &why);
  return rc == SALP_OK ? rc : fail(rc, why);
}

// What a policy of this handle is checked against and made for (salp_policy_object.h); a NULL handle: zeros.
PolicyDims policy_dims(const salp_vec* h) { return h ? PolicyDims{h->obs_dim, h->act_dim, h->kmax, h->n, h->device, h->fmax} : PolicyDims{}; }

typedef void (*reset_fn)(DevParams, DevState, const uint8_t*, float*, int);

// True when in-kernel action generation is available for this handle and output signature.
bool can_generate_in_kernel(const salp_vec* h, bool full) { return full && h->kmax == 3; }

// The unit that holds the handle's rollout kernels (fmax, kmax and std_consts are fixed at create).
// K = 3 (every preset): kernels by food-slot count, with the reference's constants as literals (STD) or — any other
// tank size, radius, drag, thrust, timing — with the constants read from the launch parameters.  K != 3 runs the
// generic instantiation (runtime constants, F <= 16, K <= 8, foods in LDS).
rollout_unit_fn rollout_unit_for(const salp_vec* h) {
  if (h->kmax != 3) return h->fmax <= 12 ? salp_rollout_generic12 : salp_rollout_generic16;
  switch (h->fmax) {
    case 1: return h->std_consts ? salp_rollout_f1_std : salp_rollout_f1_rt;
    case 4: return h->std_consts ? salp_rollout_f4_std : salp_rollout_f4_rt;
    case 8: return h->std_consts ? salp_rollout_f8_std : salp_rollout_f8_rt;
    case 12: return h->std_consts ? salp_rollout_f12_std : salp_rollout_f12_rt;
    default: return h->std_consts ? salp_rollout_f16_std : salp_rollout_f16_rt;
  }
}
template <bool STD>
reset_fn reset_kernel_k3(const salp_vec* h) {
  if (h->fmax == 1) return (reset_fn)salp_reset_kernel<1, 3, STD>;
  if (h->fmax == 4) return (reset_fn)salp_reset_kernel<4, 3, STD>;
  if (h->fmax == 8) return (reset_fn)salp_reset_kernel<8, 3, STD>;
  if (h->fmax == 12) return (reset_fn)salp_reset_kernel<12, 3, STD>;
  return (reset_fn)salp_reset_kernel<16, 3, STD>;
}
reset_fn reset_kernel_for(const salp_vec* h) {
  if (h->kmax == 3) return h->std_consts ? reset_kernel_k3<true>(h) : reset_kernel_k3<false>(h);
  return (reset_fn)salp_reset_kernel<16, 8, false>;
}

// The part of IOPtrs that every rollout call fills in the same way; the rest starts out NULL.
IOPtrs io_for(const salp_vec* h) {
  IOPtrs io = {};
  io.stats = h->stats_enabled ? h->stats : nullptr;
  io.global_step = h->global_step;
  return io;
}

#ifdef SALP_EXP_STAMPS   // experiment builds: the __device__ globals exist once per unit; read the unit that launched last
int (*g_read_stamps)(uint32_t*, int) = exp_read_stamps;
#endif
#ifdef SALP_EXP_COUNT
int (*g_read_counters)(unsigned long long*) = exp_read_counters;
#endif

// What a rollout launch writes and where its actions come from.
//   out: kOutStreams — the per-step streams of io, the signature follows from which are present;  kOutPacked — record_block(io)
//        holds transition records (kSigPacked), packed_has_final(io) asks for the terminal-observation tail;  kOutSummary —
//        record_block(io) holds summary records (kSigSummary; policy only), accumulate(io) = SALP_EVAL_ACCUMULATE;  kOutNav —
//        record_block(io) holds navigation records (kSigNav; deterministic policy, one food, forced breathing: the caller has
//        checked), accumulate(io) as for the summary, io.nav_line / nav_radius / nav_track the trial lines, the goal radius and
//        the track.  (set_record_block / set_policy_block and the readers: salp_rollout_traits.h, next to IOPtrs.)
//   act: ACT_READ — io.act, or generated in the kernel when that is NULL (only reached when can_generate_in_kernel());
//        ACT_POLICY / ACT_POLICY_SAMPLED — io.act is a policy's device block (set_policy_block) (the caller has checked K = 3 and the
//        four main outputs; ACT_POLICY_SAMPLED: a Gaussian policy, io.logp_out may be set);  ACT_POLICY_WIDE / _WIDE_SAMPLED — the same
//        two with a block of salp_policy_wide.h (policy_act(): the caller has a policy that passed the wide create)
enum { kOutStreams = 0, kOutPacked = 1, kOutSummary = 2, kOutNav = 3 };
struct RolloutKind { int out, act; };

int launch_rollout(salp_vec* h, const IOPtrs& io, int H, hipStream_t st, RolloutKind kind) {
  const bool policy = kind.act >= ACT_POLICY;
  const bool main_outputs = io.obs && io.reward && io.terminated && io.truncated;
  // (policy: final_obs / info do not exist — io.final_obs is accumulate(io), io.info's slot holds logp_out)
  const bool extras = !policy && (io.final_obs || io.info);
  const int sig = kind.out == kOutNav ? kSigNav : kind.out == kOutSummary ? kSigSummary : kind.out == kOutPacked ? kSigPacked
                : (!main_outputs ? kSigPartial : (extras ? kSigExtras : kSigMain));
  if (policy && sig != kSigMain && sig != kSigPacked && sig != kSigSummary && sig != kSigNav)
    return fail(SALP_ERR_INVALID, "policy kernels exist for the main-only, the packed, the summary and the navigation signature");
  const int gen = policy ? kind.act : (io.act == nullptr ? ACT_GEN : ACT_READ);
  // envs in full wavefronts: unpredicated kernel
  int64_t n_full = h->n / kWave * kWave;
  // A small ragged batch (step-per-launch acting loops) is launch-bound: one predicated launch over the whole
  // range instead of two; the predicates only cost when the write stream is the bound.
  if (n_full < h->n && h->n * (int64_t)H <= (int64_t)1 << 22) n_full = 0;
  // the kernel of each launch with the signature it was compiled for, which is not always `sig` (pick_sig)
  const rollout_unit_fn unit = rollout_unit_for(h);
  const bool forced = h->P.forced != 0;
  const RolloutPick none = {nullptr, -1};
  const RolloutPick full = (n_full > 0) ? unit(false, forced, sig, gen) : none;
  const RolloutPick ragged = (n_full < h->n) ? unit(true, forced, sig, gen) : none;
  const RolloutPick& first = (n_full > 0) ? full : ragged;
  if ((n_full > 0 && !full.fn) || (n_full < h->n && !ragged.fn))      // (kSigNav asked of a handle class that has no such kernel)
    return fail(SALP_ERR_INVALID, "no kernel of this output signature exists for this handle");
  h->last_sigs[0] = full.sig;
  h->last_sigs[1] = ragged.sig;
  h->last_launch[0] = h->fmax; h->last_launch[1] = h->kmax; h->last_launch[2] = (h->kmax == 3) ? h->std_consts : 0;
  h->last_wide = (gen == ACT_POLICY_WIDE || gen == ACT_POLICY_WIDE_SAMPLED) ? 1 : 0;
  // [5] keeps its two policy values: 2 deterministic, 3 sampled, whichever scheme evaluates (salp_vec_last_launch_policy_wide tells)
  h->last_launch[3] = h->P.forced; h->last_launch[4] = first.sig; h->last_launch[5] = h->last_wide ? gen - (ACT_POLICY_WIDE - ACT_POLICY) : gen;
  h->last_launch[6] = n_full; h->last_launch[7] = h->n - n_full;
  h->last_kernel = first.fn;     // the main (else the predicated) kernel
#ifdef SALP_EXP_STAMPS
  g_read_stamps = first.read_stamps;
#endif
#ifdef SALP_EXP_COUNT
  g_read_counters = first.read_counters;
#endif
  if (n_full > 0) {
    const int rc = launch_1d((rollout_fn)full.fn, n_full, kBlock, st, h->P, h->S, io, H, (int64_t)0, n_full, (const ColdBlock*)h->cold);
    if (rc != SALP_OK) return rc;
  }
  if (n_full < h->n)                                // the last n % 64 envs (or the whole small batch): predicated stores
    return launch_1d((rollout_fn)ragged.fn, h->n - n_full, kBlock, st, h->P, h->S, io, H, n_full, h->n, (const ColdBlock*)h->cold);
  return SALP_OK;
}

// What the record calls (packed, summary, navigation) check of `flags` and of a device `rec`: no bit outside `allowed`,
// and 16-byte alignment, as the kernels write a record in 16-byte stores.
int check_record_args(uint32_t flags, uint32_t allowed, const char* bits_msg, const void* rec, const char* align_msg) {
  if (flags & ~allowed) return fail(SALP_ERR_INVALID, bits_msg);
  if ((flags & SALP_DEVICE_PTRS) && ((uintptr_t)rec & 15u)) return fail(SALP_ERR_INVALID, align_msg);
  return SALP_OK;
}
const char* const kEvalFlagBits = "unknown flag bits (SALP_DEVICE_PTRS and SALP_EVAL_ACCUMULATE are defined)";

}  // namespace

// salp_policy_upload.h: shared with salp_robot.hip
hipError_t salp::policy_block_upload(const PolicyBlock& b, const float* weights, bool device_ptrs, hipStream_t st) {
  const float* src = weights;
  if (!device_ptrs) {
    const size_t pub_b = (size_t)b.n_policies * b.words * sizeof(float);
    const hipError_t e = hipMemcpyAsync(b.pub, weights, pub_b, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    src = b.pub;
  }
  const int64_t total = (int64_t)b.n_policies * b.stride;
  hipLaunchKernelGGL(salp_policy_relayout_kernel, dim3(blocks_for(total, kBlock)), dim3(kBlock), 0, st, b.block, src, b.map, b.stride,
                     b.words, total);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || device_ptrs) return e;
  return hipStreamSynchronize(st);
}

hipError_t salp::policy_noise_write(float* block, uint64_t value, bool set, hipStream_t st) {
  hipLaunchKernelGGL(salp_policy_noise_kernel, dim3(1), dim3(1), 0, st, block, set ? (uint64_t)0 : value, set ? value : (uint64_t)0, set ? 1 : 0);
  return hipGetLastError();
}

extern "C" {

const char* salp_last_error(void) { return g_err.c_str(); }
int salp_abi_version(void) { return SALP_ABI_VERSION; }

int salp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int salp_config_default(salp_config_t* c) {
  if (!c) return fail(SALP_ERR_INVALID, "cfg is NULL");
  default_config(c);     // salp_params.h
  return SALP_OK;
}

int salp_vec_create(const salp_config_t* cfg, int64_t n_envs, int device_id, uint64_t seed,
                    int64_t env_index_base, salp_vec_t** out) {
  if (!out) return fail(SALP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  int rc = validate(cfg);
  if (rc != SALP_OK) return rc;
  if (n_envs <= 0 || n_envs > ((int64_t)1 << 31) - kBlock) return fail(SALP_ERR_INVALID, "n_envs out of range");
  if (env_index_base < 0) return fail(SALP_ERR_INVALID, "env_index_base must be >= 0");
  rc = check_device_id(device_id);
  if (rc != SALP_OK) return rc;
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(device_id));

  salp_vec* h = new (std::nothrow) salp_vec();     // value-initialised: every field zero
  if (!h) return fail(SALP_ERR_OOM, "host allocation failed");
  h->last_sigs[0] = h->last_sigs[1] = -1;
  h->cfg = *cfg; h->device = device_id; h->n = n_envs; h->seed = seed; h->global_step = 0;
  h->F = cfg->num_food_items; h->K = cfg->max_observed_food;
  h->obs_dim = 10 + 4 * h->K + 2; h->act_dim = cfg->forced_breathing ? 1 : 2;
  h->kmax = (h->K == 3) ? 3 : 8;
  // food slots of the kernel instantiation: 1 (single_food*.yaml), 4, 8 (the class default of 5 foods), 12 (sac_gail.yaml), 16
  h->fmax = (h->kmax == 3) ? (h->F <= 1 ? 1 : (h->F <= 4 ? 4 : (h->F <= 8 ? 8 : (h->F <= 12 ? 12 : 16)))) : (h->F <= 12 ? 12 : 16);
  const int64_t pitch = (int64_t)align_up((size_t)n_envs, 64);
  h->P = make_params(*cfg, n_envs, pitch, seed, env_index_base);
  h->std_consts = is_std(h->P) ? 1 : 0;
  h->nf_rows = (size_t)(SF_FOOD0 + 2 * h->F);
  h->stats_enabled = 1;

  // allocations, the cold block's copy and the memsets as one chain: `stage` names the step that failed
  const size_t f_bytes = h->nf_rows * (size_t)pitch * sizeof(double), i_bytes = (size_t)SI_COUNT * (size_t)pitch * sizeof(int32_t);
  const char* stage = "hipMalloc(state): ";
  hipError_t e = hipMalloc((void**)&h->S.f, f_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&h->S.i, i_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&h->stats, SALP_STATS_REPLICAS * sizeof(DevStats));
  if (e == hipSuccess) {
    stage = "hipMalloc/hipMemcpy(cold block): ";
    e = hipMalloc((void**)&h->cold, sizeof(ColdBlock));
  }
  if (e == hipSuccess) {
    h->P.seed = (seed_word_t*)(uintptr_t)h->cold->seed;   // device address; the kernels read the key words through it
    h->P.self = (dev_params_c*)(uintptr_t)&h->cold->P;    // likewise the constants of the STD = false kernels
    ColdBlock cb;
    cb.P = h->P; cb.S = h->S;
    cb.seed[0] = (uint32_t)seed; cb.seed[1] = (uint32_t)(seed >> 32);
    e = hipMemcpy(h->cold, &cb, sizeof(cb), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) {
    stage = "hipMemset(state): ";
    e = hipMemset(h->S.f, 0, f_bytes);
  }
  if (e == hipSuccess) e = hipMemset(h->S.i, 0, i_bytes);
  if (e == hipSuccess) e = hipMemset(h->stats, 0, SALP_STATS_REPLICAS * sizeof(DevStats));
  if (e != hipSuccess) {
    const std::string m = std::string(stage) + hipGetErrorString(e);
    salp_vec_destroy(h);
    return fail(e == hipErrorOutOfMemory ? SALP_ERR_OOM : SALP_ERR_HIP, m);
  }
  // initial reset of every env (consumes the first draws of each env's stream)
  rc = salp_vec_reset(h, nullptr, nullptr, SALP_DEVICE_PTRS, nullptr);
  if (rc == SALP_OK) {   // the handle's own work only (the null stream it was issued on), not a device-wide drain
    hipError_t es = hipStreamSynchronize(nullptr);
    if (es != hipSuccess) rc = fail(SALP_ERR_HIP, std::string("initial reset: ") + hipGetErrorString(es));
  }
  if (rc != SALP_OK) { std::string m = g_err; salp_vec_destroy(h); g_err = m; return rc; }
  *out = h;
  return SALP_OK;
}

void salp_vec_destroy(salp_vec_t* h) {
  if (!h) return;
  DeviceScope dev_scope;
  (void)dev_scope.enter(h->device);
  (void)hipStreamSynchronize(h->last_stream);     // hipFree does not wait for kernels on non-blocking streams
  if (h->S.f) (void)hipFree(h->S.f);
  if (h->S.i) (void)hipFree(h->S.i);
  if (h->stats) (void)hipFree(h->stats);
  if (h->cold) (void)hipFree(h->cold);
  if (h->act_buf) (void)hipFree(h->act_buf);
  delete h;     // the staging block goes with it
}

int64_t salp_vec_num_envs(const salp_vec_t* h) { return h ? h->n : 0; }
int salp_vec_obs_dim(const salp_vec_t* h) { return h ? h->obs_dim : 0; }
int salp_vec_act_dim(const salp_vec_t* h) { return h ? h->act_dim : 0; }
#ifdef SALP_EXP_STAMPS
// experiment build only: the per-wavefront phase cycle sums of the last rollout launches (16 words per wavefront)
int salp_exp_read_stamps(uint32_t* dst, int words) { return g_read_stamps(dst, words); }
#endif
#ifdef SALP_EXP_COUNT
int salp_exp_read_counters(unsigned long long* dst) { return g_read_counters(dst); }
#endif
int salp_vec_num_food(const salp_vec_t* h) { return h ? h->F : 0; }
int salp_vec_device(const salp_vec_t* h) { return h ? h->device : -1; }
int64_t salp_vec_global_step(const salp_vec_t* h) { return h ? h->global_step : 0; }
int salp_vec_last_launch(const salp_vec_t* h, int64_t info[8]) {
  if (!h || !info) return fail(SALP_ERR_INVALID, "handle/info is NULL");
  memcpy(info, h->last_launch, sizeof(h->last_launch));
  return SALP_OK;
}

int salp_vec_last_launch_signatures(const salp_vec_t* h, int64_t sig[2]) {
  if (!h || !sig) return fail(SALP_ERR_INVALID, "handle/sig is NULL");
  sig[0] = h->last_sigs[0]; sig[1] = h->last_sigs[1];
  return SALP_OK;
}

int salp_vec_last_kernel_resources(const salp_vec_t* h, int32_t info[4]) {
  if (!h || !info) return fail(SALP_ERR_INVALID, "handle/info is NULL");
  if (!h->last_kernel) return fail(SALP_ERR_INVALID, "no step / rollout call has been issued on this handle");
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(h->device));
  hipFuncAttributes attr;
  HIP_TRY(hipFuncGetAttributes(&attr, h->last_kernel));
  int blocks = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, h->last_kernel, kBlock, 0));
  info[0] = attr.numRegs; info[1] = (int32_t)attr.sharedSizeBytes; info[2] = (int32_t)attr.localSizeBytes; info[3] = blocks;
  return SALP_OK;
}

int salp_vec_set_base_num_food(salp_vec_t* h, int32_t k) {
  if (!h) return fail(SALP_ERR_INVALID, "handle is NULL");
  if (k < 0 || k > h->P.F) return fail(SALP_ERR_INVALID, "base_num_food_items must be within 0..num_food_items of the handle");
  h->P.F_base = k;     // kernel parameters are passed by value at every launch
  return SALP_OK;
}
int32_t salp_vec_base_num_food(const salp_vec_t* h) { return h ? h->P.F_base : 0; }

// reset (do_reset = 1, every env or those of `mask`) and observe (do_reset = 0): one kernel
static int reset_impl(salp_vec_t* h, const uint8_t* mask, float* obs, int do_reset, uint32_t flags, void* stream) {
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  HostStream s[] = {stream_out(obs, (size_t)h->n * h->obs_dim), stream_in(mask, (size_t)h->n)};
  return staged(h->stage, f.st, flags & SALP_DEVICE_PTRS, s, [&] {
    return launch_1d(reset_kernel_for(h), h->n, kBlock, f.st, h->P, h->S, s[1].as<const uint8_t>(), s[0].as<float>(), do_reset);
  });
}

int salp_vec_reset(salp_vec_t* h, const uint8_t* mask, float* obs, uint32_t flags, void* stream) {
  if (!h) return fail(SALP_ERR_INVALID, "handle is NULL");
  return reset_impl(h, mask, obs, 1, flags, stream);
}

int salp_vec_observe(salp_vec_t* h, float* obs, uint32_t flags, void* stream) {
  if (!h || !obs) return fail(SALP_ERR_INVALID, "handle/obs is NULL");
  return reset_impl(h, nullptr, obs, 0, flags, stream);
}

// Behind the launches of a sampled call: the policy's noise step goes on by the call's horizon, on the device (a replayed
// graph draws fresh noise).  The policy arrives const (the entry points' signature), yet this writes its noise word in
// device memory and its last_stream (`mutable`): include/salp_vec.h says so.  Should this one-thread launch fail, the
// rollout kernels are already enqueued: the call then returns the error with the envs stepped and the global step advanced
// but the noise step where it was — the caller must set it (salp_policy_set_noise_step) before sampling on.
static int advance_noise(const salp_policy_t* pol, int H, hipStream_t st) {
  pol->last_stream = st;
  return policy_noise_advance(pol->block, H, st);
}

// Device-generated actions of the next H steps into act_out when given, else into the handle's own buffer (grown on demand).
static int generate_actions(salp_vec_t* h, int32_t H, float* act_out, hipStream_t st, const float** act) {
  float* dst = act_out;
  if (!dst) {
    const size_t need_a = (size_t)H * (size_t)h->n * h->act_dim * sizeof(float);
    if (need_a > h->act_bytes) {
      if (h->act_buf) { (void)hipFree(h->act_buf); h->act_buf = nullptr; h->act_bytes = 0; }
      HIP_TRY(hipMalloc((void**)&h->act_buf, need_a));
      h->act_bytes = need_a;
    }
    dst = h->act_buf;
  }
  *act = dst;
  return launch_1d(salp_gen_actions_kernel, h->n, kBlock, st, h->P, dst, (int)H, h->act_dim, (int64_t)h->global_step);
}

// The launches of a rollout call and what follows them when they succeed: the global step goes on by the horizon and, for
// a sampled call, so does the policy's noise step (advance_noise) — in the host-pointer form both before the copies out.
static int run_rollout(salp_vec_t* h, const IOPtrs& io, int32_t H, hipStream_t st, RolloutKind kind, const salp_policy_t* pol = nullptr) {
  const int rc = launch_rollout(h, io, H, st, kind);
  if (rc != SALP_OK) return rc;
  h->global_step += H;
  return (kind.act == ACT_POLICY_SAMPLED || kind.act == ACT_POLICY_WIDE_SAMPLED) ? advance_noise(pol, H, st) : SALP_OK;
}

static int rollout_impl(salp_vec_t* h, const float* act, int32_t H, float* obs, float* reward,
                        uint8_t* terminated, uint8_t* truncated, float* final_obs, int32_t* info,
                        float* act_out, uint32_t flags, void* stream) {
  if (!h) return fail(SALP_ERR_INVALID, "handle is NULL");
  if (H <= 0) return fail(SALP_ERR_INVALID, "horizon must be >= 1");
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  const bool device_ptrs = (flags & SALP_DEVICE_PTRS) != 0;
  IOPtrs io = io_for(h);
  // final_obs goes in as well as out (the rows of unfinished envs stay as they are)
  const size_t HN = (size_t)H * (size_t)h->n;
  HostStream s[] = {act ? stream_in(act, HN * h->act_dim) : stream_out(act_out, HN * h->act_dim),
                    stream_out(obs, HN * h->obs_dim), stream_out(final_obs, HN * h->obs_dim, true), stream_out(reward, HN),
                    stream_out(terminated, HN), stream_out(truncated, HN), stream_out(info, HN * SALP_INFO_COLS)};
  return staged(h->stage, f.st, device_ptrs, s, [&] {
    io.obs = s[1].as<float>(); io.final_obs = s[2].as<float>(); io.reward = s[3].as<float>();
    io.terminated = s[4].as<uint8_t>(); io.truncated = s[5].as<uint8_t>(); io.info = s[6].as<int32_t>();
    // The actions are where the two forms differ.  Device pointers: act and act_out are two arrays (the kernel writes the
    // actions it took to act_out), and with no act the actions are generated in the kernel where such a kernel exists.
    // Host pointers: with no act they are always generated ahead of the launch (never in the kernel), into act_out's
    // staging when that is wanted, and the kernel has no act_out.
    if (device_ptrs) {
      io.act = act; io.act_out = act_out;
      const bool full_sig = io.obs && io.reward && io.terminated && io.truncated && !io.final_obs && !io.info;
      if (!act && !can_generate_in_kernel(h, full_sig)) {
        const int rc = generate_actions(h, H, act_out, f.st, &io.act);
        if (rc != SALP_OK) return rc;
      }
    } else {
      io.act = s[0].as<float>();
      if (!act) {
        const int rc = generate_actions(h, H, s[0].as<float>(), f.st, &io.act);
        if (rc != SALP_OK) return rc;
      }
    }
    return run_rollout(h, io, H, f.st, {kOutStreams, ACT_READ});
  });
}

int salp_vec_step(salp_vec_t* h, const float* act, float* obs, float* reward, uint8_t* terminated,
                  uint8_t* truncated, float* final_obs, int32_t* info, uint32_t flags, void* stream) {
  if (!act) return fail(SALP_ERR_INVALID, "act is NULL");
  return rollout_impl(h, act, 1, obs, reward, terminated, truncated, final_obs, info, nullptr, flags, stream);
}

int salp_vec_rollout(salp_vec_t* h, const float* act, int32_t horizon, float* obs, float* reward,
                     uint8_t* terminated, uint8_t* truncated, float* final_obs, float* act_out,
                     uint32_t flags, void* stream) {
  return rollout_impl(h, act, horizon, obs, reward, terminated, truncated, final_obs, nullptr, act_out, flags, stream);
}

int salp_vec_record_width(const salp_vec_t* h, uint32_t flags) {
  if (!h) return 0;
  return h->obs_dim + SALP_REC_EXTRA_COLS + ((flags & SALP_REC_FINAL_OBS) ? h->obs_dim : 0);
}

// salp_vec_step_packed / salp_vec_rollout_packed: the kSigPacked kernels.  Everything is checked before anything is launched.
static int packed_impl(salp_vec_t* h, const float* act, int32_t H, float* rec, float* act_out, uint32_t flags, void* stream) {
  if (!h) return fail(SALP_ERR_INVALID, "handle is NULL");
  if (!rec) return fail(SALP_ERR_INVALID, "rec is NULL");
  if (H <= 0) return fail(SALP_ERR_INVALID, "horizon must be >= 1");
  if (const int rc = check_record_args(flags, SALP_DEVICE_PTRS | SALP_REC_FINAL_OBS,
                                       "unknown flag bits (SALP_DEVICE_PTRS and SALP_REC_FINAL_OBS are defined)", rec,
                                       "rec must be 16-byte aligned (the records are written as float4)"))
    return rc;
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  const bool with_final = (flags & SALP_REC_FINAL_OBS) != 0;
  IOPtrs io = io_for(h);
  // s[0]: the actions, or — none given — where generated ones go (act_out; NULL: the handle's buffer)
  const size_t HN = (size_t)H * (size_t)h->n;
  HostStream s[] = {act ? stream_in(act, HN * h->act_dim) : stream_out(act_out, HN * h->act_dim),
                    stream_out(rec, HN * (size_t)salp_vec_record_width(h, flags), with_final)};   // in: the tails of unfinished rows stay as they are
  return staged(h->stage, f.st, flags & SALP_DEVICE_PTRS, s, [&] {
    io.act = s[0].as<float>(); set_record_block(io, s[1].as<float>(), with_final);
    if (!act) {
      const int rc = generate_actions(h, H, s[0].as<float>(), f.st, &io.act);
      if (rc != SALP_OK) return rc;
    }
    return run_rollout(h, io, H, f.st, {kOutPacked, ACT_READ});
  });
}

int salp_vec_step_packed(salp_vec_t* h, const float* act, float* rec, uint32_t flags, void* stream) {
  if (!act) return fail(SALP_ERR_INVALID, "act is NULL");
  return packed_impl(h, act, 1, rec, nullptr, flags, stream);
}

int salp_vec_rollout_packed(salp_vec_t* h, const float* act, int32_t horizon, float* rec, float* act_out,
                            uint32_t flags, void* stream) {
  return packed_impl(h, act, horizon, rec, act_out, flags, stream);
}

// The policy object's calls: salp_policy_object.h.
int salp_policy_words(const salp_vec_t* h, const salp_policy_desc_t* desc) { return policy_words(policy_dims(h), desc, false); }
int salp_policy_words_gaussian(const salp_vec_t* h, const salp_policy_desc_t* desc) { return policy_words(policy_dims(h), desc, true); }

static int policy_create_impl(salp_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags, void* stream,
                              salp_policy_t** out, bool gaussian, bool wide = false) {
  // of `flags`, create and update read bit 0 (SALP_DEVICE_PTRS) and ignore the rest: every bit is a known one
  const int rc = policy_create(policy_dims(h), desc, weights, flags, ~0u, stream, gaussian, out, wide);
  if (rc == SALP_OK) (*out)->h = h;
  return rc;
}

int salp_policy_create(salp_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags, void* stream,
                       salp_policy_t** out) {
  return policy_create_impl(h, desc, weights, flags, stream, out, false);
}

int salp_policy_create_gaussian(salp_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags, void* stream,
                                salp_policy_t** out) {
  return policy_create_impl(h, desc, weights, flags, stream, out, true);
}

// include/salp_vec_policy_wide.h: the same object with the ranges and the block of salp_policy_wide.h
int salp_policy_words_wide(const salp_vec_t* h, const salp_policy_desc_t* desc, int gaussian) {
  return policy_words(policy_dims(h), desc, gaussian != 0, true);
}

int salp_policy_create_wide(salp_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags, void* stream,
                            salp_policy_t** out) {
  return policy_create_impl(h, desc, weights, flags, stream, out, false, true);
}

int salp_policy_create_gaussian_wide(salp_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags, void* stream,
                                     salp_policy_t** out) {
  return policy_create_impl(h, desc, weights, flags, stream, out, true, true);
}

int salp_vec_last_launch_policy_wide(const salp_vec_t* h) { return h ? h->last_wide : 0; }

void salp_policy_destroy(salp_policy_t* pol) {
  if (pol) policy_free(pol, &pol->h->last_stream);     // its own uploads, and the handle's launches that read the block
}

int salp_policy_update(salp_policy_t* pol, const float* weights, uint32_t flags, void* stream) {
  if (!pol || !weights) return fail(SALP_ERR_INVALID, "policy/weights is NULL");
  return policy_update(*pol, weights, (flags & SALP_DEVICE_PTRS) != 0, stream);
}

int salp_policy_set_noise_step(salp_policy_t* pol, uint64_t n, void* stream) {
  if (!pol) return fail(SALP_ERR_INVALID, "policy is NULL");
  return policy_set_noise_step(*pol, n, stream);
}

int salp_policy_noise_step(salp_policy_t* pol, uint64_t* n) {
  if (!pol || !n) return fail(SALP_ERR_INVALID, "policy/n is NULL");
  return policy_noise_step(*pol, n);
}

// What every call that runs a policy checks first.  (The descriptor cannot fail once the policy is known to be the handle's:
// it passed at create with the same handle.  Its check is kept as the guard of the kernels' K = 3 and one-policy-per-wavefront
// rules.)
static int check_policy_call(const salp_vec_t* h, const salp_policy_t* pol, bool sampled) {
  if (!h || !pol) return fail(SALP_ERR_INVALID, "handle/policy is NULL");
  if (sampled && !pol->gaussian) return fail(SALP_ERR_INVALID, "sampling needs a Gaussian policy (salp_policy_create_gaussian)");
  if (pol->h != h || pol->device != h->device || pol->obs_dim != h->obs_dim || pol->act_dim != h->act_dim || pol->n != h->n)
    return fail(SALP_ERR_INVALID, "the policy belongs to another handle (or other dimensions)");
  return check_policy_dims(policy_dims(h), &pol->d, pol->gaussian != 0, nullptr, pol->wide != 0);
}
// The action source of a policy call: the policy's scheme (salp_policy.h or salp_policy_wide.h), deterministic or sampling.
static int policy_act(const salp_policy_t* pol, bool sampled) {
  return pol->wide ? (sampled ? ACT_POLICY_WIDE_SAMPLED : ACT_POLICY_WIDE) : (sampled ? ACT_POLICY_SAMPLED : ACT_POLICY);
}

// salp_vec_rollout_policy (sampled = false, logp_out = NULL) and salp_vec_rollout_policy_sampled
static int rollout_policy_impl(salp_vec_t* h, const salp_policy_t* pol, int32_t H, float* obs, float* reward, uint8_t* terminated,
                               uint8_t* truncated, float* act_out, float* logp_out, uint32_t flags, void* stream, bool sampled) {
  int rc = check_policy_call(h, pol, sampled);
  if (rc != SALP_OK) return rc;
  if (H <= 0) return fail(SALP_ERR_INVALID, "horizon must be >= 1");
  if (!obs || !reward || !terminated || !truncated)
    return fail(SALP_ERR_INVALID, "obs, reward, terminated and truncated are all required");
  CallFrame f;
  if ((rc = f.enter(h, stream)) != SALP_OK) return rc;
  IOPtrs io = io_for(h);
  set_policy_block(io, pol->block);
  const size_t HN = (size_t)H * (size_t)h->n;
  HostStream s[] = {stream_out(obs, HN * h->obs_dim), stream_out(reward, HN), stream_out(terminated, HN), stream_out(truncated, HN),
                    stream_out(act_out, HN * h->act_dim), stream_out(sampled ? logp_out : nullptr, HN)};
  return staged(h->stage, f.st, flags & SALP_DEVICE_PTRS, s, [&] {
    io.obs = s[0].as<float>(); io.reward = s[1].as<float>(); io.terminated = s[2].as<uint8_t>(); io.truncated = s[3].as<uint8_t>();
    io.act_out = s[4].as<float>();
    if (sampled) io.logp_out = s[5].as<float>();
    return run_rollout(h, io, H, f.st, {kOutStreams, policy_act(pol, sampled)}, pol);
  });
}

int salp_vec_rollout_policy(salp_vec_t* h, const salp_policy_t* pol, int32_t H, float* obs, float* reward,
                            uint8_t* terminated, uint8_t* truncated, float* act_out, uint32_t flags, void* stream) {
  return rollout_policy_impl(h, pol, H, obs, reward, terminated, truncated, act_out, nullptr, flags, stream, false);
}

int salp_vec_rollout_policy_sampled(salp_vec_t* h, const salp_policy_t* pol, int32_t H, float* obs, float* reward,
                                    uint8_t* terminated, uint8_t* truncated, float* act_out, float* logp_out,
                                    uint32_t flags, void* stream) {
  return rollout_policy_impl(h, pol, H, obs, reward, terminated, truncated, act_out, logp_out, flags, stream, true);
}

// salp_vec_rollout_policy_packed (and _sampled; include/salp_vec_policy_packed.h): the kSigPacked kernels with the in-kernel
// policy — the checks of the policy calls, then those of the packed calls; everything before anything is launched.
static int rollout_policy_packed_impl(salp_vec_t* h, const salp_policy_t* pol, int32_t H, float* rec, float* act_out, float* logp_out,
                                      uint32_t flags, void* stream, bool sampled) {
  int rc = check_policy_call(h, pol, sampled);
  if (rc != SALP_OK) return rc;
  if (!rec) return fail(SALP_ERR_INVALID, "rec is NULL");
  if (H <= 0) return fail(SALP_ERR_INVALID, "horizon must be >= 1");
  rc = check_record_args(flags, SALP_DEVICE_PTRS | SALP_REC_FINAL_OBS,
                         "unknown flag bits (SALP_DEVICE_PTRS and SALP_REC_FINAL_OBS are defined)", rec,
                         "rec must be 16-byte aligned (the records are written as float4)");
  if (rc != SALP_OK) return rc;
  CallFrame f;
  if ((rc = f.enter(h, stream)) != SALP_OK) return rc;
  const bool with_final = (flags & SALP_REC_FINAL_OBS) != 0;
  IOPtrs io = io_for(h);
  set_policy_block(io, pol->block);
  const size_t HN = (size_t)H * (size_t)h->n;
  HostStream s[] = {stream_out(rec, HN * (size_t)salp_vec_record_width(h, flags), with_final),   // in: the tails of unfinished rows stay as they are
                    stream_out(act_out, HN * h->act_dim), stream_out(sampled ? logp_out : nullptr, HN)};
  return staged(h->stage, f.st, flags & SALP_DEVICE_PTRS, s, [&] {
    set_record_block(io, s[0].as<float>(), with_final);
    io.act_out = s[1].as<float>();
    if (sampled) io.logp_out = s[2].as<float>();     // (the info slot: the record carries the counters)
    return run_rollout(h, io, H, f.st, {kOutPacked, policy_act(pol, sampled)}, pol);
  });
}

int salp_vec_rollout_policy_packed(salp_vec_t* h, const salp_policy_t* pol, int32_t horizon, float* rec, float* act_out,
                                   uint32_t flags, void* stream) {
  return rollout_policy_packed_impl(h, pol, horizon, rec, act_out, nullptr, flags, stream, false);
}

int salp_vec_rollout_policy_packed_sampled(salp_vec_t* h, const salp_policy_t* pol, int32_t horizon, float* rec, float* act_out,
                                           float* logp_out, uint32_t flags, void* stream) {
  return rollout_policy_packed_impl(h, pol, horizon, rec, act_out, logp_out, flags, stream, true);
}

// salp_vec_evaluate_policy (and _sampled): the kSigSummary kernels.  Everything is checked before anything is launched.
static int evaluate_policy_impl(salp_vec_t* h, const salp_policy_t* pol, int32_t H, void* rec, uint32_t flags, void* stream, bool sampled) {
  int rc = check_policy_call(h, pol, sampled);
  if (rc != SALP_OK) return rc;
  if (!rec) return fail(SALP_ERR_INVALID, "rec is NULL");
  if (H <= 0) return fail(SALP_ERR_INVALID, "horizon must be >= 1");
  rc = check_record_args(flags, SALP_DEVICE_PTRS | SALP_EVAL_ACCUMULATE, kEvalFlagBits, rec,
                         "rec must be 16-byte aligned (a record is written as two 16-byte stores)");
  if (rc != SALP_OK) return rc;
  CallFrame f;
  if ((rc = f.enter(h, stream)) != SALP_OK) return rc;
  const bool accumulate = (flags & SALP_EVAL_ACCUMULATE) != 0;
  IOPtrs io = io_for(h);
  set_policy_block(io, pol->block);
  HostStream s[] = {stream_out((int32_t*)rec, (size_t)h->n * SALP_EVAL_WORDS, accumulate)};
  return staged(h->stage, f.st, flags & SALP_DEVICE_PTRS, s, [&] {
    set_record_block(io, s[0].as<float>(), accumulate);
    return run_rollout(h, io, H, f.st, {kOutSummary, policy_act(pol, sampled)}, pol);
  });
}

int salp_vec_evaluate_policy(salp_vec_t* h, const salp_policy_t* pol, int32_t H, void* rec, uint32_t flags, void* stream) {
  return evaluate_policy_impl(h, pol, H, rec, flags, stream, false);
}

int salp_vec_evaluate_policy_sampled(salp_vec_t* h, const salp_policy_t* pol, int32_t H, void* rec, uint32_t flags, void* stream) {
  return evaluate_policy_impl(h, pol, H, rec, flags, stream, true);
}

// salp_vec_evaluate_navigation: the kSigNav kernels.  Everything is checked before anything is launched.
int salp_vec_evaluate_navigation(salp_vec_t* h, const salp_policy_t* pol, int32_t H, const double* line, double goal_radius,
                                 void* rec, double* track, uint32_t flags, void* stream) {
  int rc = check_policy_call(h, pol, false);
  if (rc != SALP_OK) return rc;
  if (h->P.autoreset) return fail(SALP_ERR_INVALID, "navigation trials need a handle with no_autoreset (nothing ends a trial but the goal)");
  if (h->cfg.num_food_items != 1 || h->fmax != 1) return fail(SALP_ERR_INVALID, "navigation trials need num_food_items == 1 (the goal)");
  if (!h->P.forced) return fail(SALP_ERR_INVALID, "navigation trials need forced breathing");
  if (!rec || !line) return fail(SALP_ERR_INVALID, "rec/line is NULL");
  if (H <= 0) return fail(SALP_ERR_INVALID, "horizon must be >= 1");
  if (!(goal_radius > 0.0) || !(goal_radius <= 1.7976931348623157e308)) return fail(SALP_ERR_INVALID, "goal_radius must be finite and positive");
  rc = check_record_args(flags, SALP_DEVICE_PTRS | SALP_EVAL_ACCUMULATE, kEvalFlagBits, rec,
                         "rec must be 16-byte aligned (a record is written as five 16-byte stores)");
  if (rc != SALP_OK) return rc;
  if ((flags & SALP_DEVICE_PTRS) && ((((uintptr_t)line) | ((uintptr_t)track)) & 15u))
    return fail(SALP_ERR_INVALID, "line and track must be 16-byte aligned (read / written 16 bytes at a time)");
  CallFrame f;
  if ((rc = f.enter(h, stream)) != SALP_OK) return rc;
  const bool accumulate = (flags & SALP_EVAL_ACCUMULATE) != 0;
  IOPtrs io = io_for(h);
  set_policy_block(io, pol->block);
  io.nav_radius = goal_radius;       // (shares its bytes with global_step, which only generated actions read)
  HostStream s[] = {stream_in(line, (size_t)h->n * 4), stream_out((int32_t*)rec, (size_t)h->n * SALP_NAV_WORDS, accumulate),
                    stream_out(track, (size_t)H * (size_t)h->n * 2)};
  return staged(h->stage, f.st, flags & SALP_DEVICE_PTRS, s, [&] {
    io.nav_line = s[0].as<const double>(); set_record_block(io, s[1].as<float>(), accumulate); io.nav_track = s[2].as<double>();
    return run_rollout(h, io, H, f.st, {kOutNav, policy_act(pol, false)}, pol);
  });
}

int salp_vec_get_state(salp_vec_t* h, double* f64, int32_t* i32, uint32_t flags, void* stream) {
  if (!h) return fail(SALP_ERR_INVALID, "handle is NULL");
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  HostStream s[] = {stream_out(f64, (size_t)SALP_F_COUNT(h->F) * h->n), stream_out(i32, (size_t)SALP_I_COUNT * h->n)};
  return staged(h->stage, f.st, flags & SALP_DEVICE_PTRS, s, [&] {
    return launch_1d(salp_get_state_kernel, h->n, kBlock, f.st, h->P, h->S, s[0].as<double>(), s[1].as<int32_t>());
  });
}

int salp_vec_set_state(salp_vec_t* h, const double* f64, const int32_t* i32, uint32_t flags, void* stream) {
  if (!h) return fail(SALP_ERR_INVALID, "handle is NULL");
  if (!(flags & SALP_DEVICE_PTRS)) {     // a host snapshot's ranges (salp_params.h): nothing is written when any env is out of range
    char msg[200];
    const int bad = check_snapshot(h->n, f64, i32, msg, sizeof msg);
    if (bad != SALP_OK) return fail(bad, msg);
  }
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  HostStream s[] = {stream_in(f64, (size_t)SALP_F_COUNT(h->F) * h->n), stream_in(i32, (size_t)SALP_I_COUNT * h->n)};
  return staged(h->stage, f.st, flags & SALP_DEVICE_PTRS, s, [&] {
    return launch_1d(salp_set_state_kernel, h->n, kBlock, f.st, h->P, h->S, s[0].as<const double>(), s[1].as<const int32_t>());
  });
}

int salp_vec_get_stats(salp_vec_t* h, salp_stats_t* out) {
  if (!h || !out) return fail(SALP_ERR_INVALID, "handle/out is NULL");
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(h->device));
  // The totals are complete once the handle's most recent launch is: wait for ITS stream (in-order), not for the
  // device — a device-wide drain here would also stall every other stream of the process (RCCL collectives in flight).
  DevStats host[SALP_STATS_REPLICAS];
  HIP_TRY(hipMemcpyAsync(host, h->stats, sizeof(host), hipMemcpyDeviceToHost, h->last_stream));
  HIP_TRY(hipStreamSynchronize(h->last_stream));
  long long acc[16] = {0};
  for (int r = 0; r < SALP_STATS_REPLICAS; ++r)
    for (int k = 0; k < 16; ++k) acc[k] += (long long)host[r].v[k];
  out->env_steps = acc[ST_STEPS]; out->episodes = acc[ST_EPISODES]; out->terminated = acc[ST_TERM];
  out->truncated = acc[ST_TRUNC]; out->collisions = acc[ST_COLL]; out->food_collected = acc[ST_FOOD];
  out->episode_length_sum = acc[ST_EPLEN];
  out->reward_sum = (double)acc[ST_REWARD] / SALP_FIXED_SCALE;
  out->episode_return_sum = (double)acc[ST_EPRET] / SALP_FIXED_SCALE;
  return SALP_OK;
}

int salp_vec_clear_stats(salp_vec_t* h) {
  if (!h) return fail(SALP_ERR_INVALID, "handle is NULL");
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(h->device));
  // stream-ordered behind the handle's most recent launch: no host synchronisation at all
  HIP_TRY(hipMemsetAsync(h->stats, 0, SALP_STATS_REPLICAS * sizeof(DevStats), h->last_stream));
  return SALP_OK;
}

int salp_vec_reseed(salp_vec_t* h, uint64_t seed, float* obs, uint32_t flags, void* stream) {
  if (!h) return fail(SALP_ERR_INVALID, "handle is NULL");
  CallFrame f;
  if (int rc = f.enter(h, stream)) return rc;
  const int64_t pitch = h->P.pitch;
  const int rc = launch_1d(salp_reseed_kernel, pitch, kBlock, f.st, h->cold, h->stats, pitch, (int)h->nf_rows, (uint32_t)seed,
                           (uint32_t)(seed >> 32));
  if (rc != SALP_OK) return rc;
  h->seed = seed;
  h->global_step = 0;
  return salp_vec_reset(h, nullptr, obs, flags, stream);   // every env, from draw counter 0 of the new streams
}

// Test support (salp_snake_math_probe.h): one of the snake step's math primitives over host arrays, staged like the other
// host-pointer calls.  The thrust forms get the launch parameters a handle of this config would have; the key words and the
// memory copy of the parameters sit in a ColdBlock of the call's own, behind the arrays in the staging block.
int salp_snake_math_probe(int device_id, int function, const salp_config_t* cfg, uint64_t seed, const double* in, double* out,
                          int64_t n) {
  if (!in || !out) return fail(SALP_ERR_INVALID, "in / out is NULL");
  if (n < 1 || n > ((int64_t)1 << 24)) return fail(SALP_ERR_INVALID, "n must be in [1, 2^24]");
  size_t rows_in = 1, rows_out = 1;
  switch (function) {
    case SALP_SNAKE_MATH_SINCOS_T: rows_out = 2; break;
    case SALP_SNAKE_MATH_SIN_NOZZLE_T: case SALP_SNAKE_MATH_COS_WRAPPED: break;
    case SALP_SNAKE_MATH_ATAN2: case SALP_SNAKE_MATH_ATAN2_PRECISE: case SALP_SNAKE_MATH_U53: rows_in = 2; break;
    case SALP_SNAKE_MATH_REL_HEADING: case SALP_SNAKE_MATH_REL_HEADING_PRECISE: rows_in = 3; break;
    case SALP_SNAKE_MATH_PHILOX: rows_in = 6; rows_out = 4; break;
    case SALP_SNAKE_MATH_THRUST_STD: case SALP_SNAKE_MATH_THRUST_RT: rows_in = 7; rows_out = 7; break;
    default: return fail(SALP_ERR_INVALID, "unknown function code");
  }
  salp_config_t c;
  if (cfg) c = *cfg; else default_config(&c);
  int rc = validate(&c);
  if (rc != SALP_OK) return rc;
  ColdBlock cb;
  memset(&cb, 0, sizeof(cb));
  cb.P = make_params(c, n, n, seed, 0);
  cb.seed[0] = (uint32_t)seed; cb.seed[1] = (uint32_t)(seed >> 32);
  if (function == SALP_SNAKE_MATH_THRUST_STD && !is_std(cb.P))
    return fail(SALP_ERR_INVALID, "THRUST_STD needs a config whose constants are the literals (the product runs it through the runtime-constant kernels)");
  rc = check_device_id(device_id);
  if (rc != SALP_OK) return rc;
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(device_id));
  StageBuffer stage;     // the call's own, released on return
  HostStream s[] = {stream_in(in, rows_in * (size_t)n), stream_out(out, rows_out * (size_t)n), stream_in(&cb, 1)};
  return staged(stage, nullptr, false, s, [&] {
    DevParams P = cb.P;
    ColdBlock* const dev = s[2].as<ColdBlock>();
    P.seed = (seed_word_t*)(uintptr_t)dev->seed;      // device addresses, as salp_vec_create sets them
    P.self = (dev_params_c*)(uintptr_t)&dev->P;
    return launch_1d(salp_snake_math_probe_kernel, n, kBlock, nullptr, P, function, s[0].as<const double>(), s[1].as<double>(), n);
  });
}

}  // extern "C"
