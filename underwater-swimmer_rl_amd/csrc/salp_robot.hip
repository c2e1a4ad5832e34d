// salp_robot.hip — the C ABI of include/salp_robot.h, include/salp_robot_rollout.h, include/salp_robot_sampled.h and
// include/salp_robot_evaluate.h, the batched HEAD simulator for gfx950: the
// reference's `Robot.step_through_cycle` (src/salp/environments/robot.py) under `SalpRobotEnv.step/reset`
// (src/salp/environments/salp_robot_env.py), one robot per lane.  Host code only: the handle and the entry points.
//   salp_robot_kernels.h   every kernel this file launches (and the notes on how the simulator is laid out on the GPU)
//   salp_robot_params.h    RobotParams and its derivation from a config, the constants, every argument check
//   salp_host.h            fail, HIP_TRY, DeviceScope, check_device_id, CallFrame, launch_1d, StageBuffer, staged()
//   salp_policy.h          the in-kernel policy's descriptor ranges, block map and header (host functions, generic in the dimensions)
//   salp_policy_object.h   the policy object behind a salp_robot_policy_t and its whole life, shared with salp_vec.hip
//   salp_policy_upload.h   the upload of a policy's weights and the write of its noise step: kernels of salp_vec.hip's unit
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>

#include <new>
#include <string>
#include <vector>

#include "../../include/salp_robot.h"
#include "../../include/salp_robot_rollout.h"
#include "../../include/salp_robot_sampled.h"
#include "../../include/salp_robot_evaluate.h"
#include "salp_robot_params.h"
#include "salp_robot_kernels.h"
#include "salp_host.h"
#include "salp_policy_object.h"

using namespace salp;

struct salp_robot_vec {
  salp_robot_config_t cfg;
  RobotParams P;
  RobotState S;
  int device;
  int64_t n;
  StageBuffer stage;  // staging for host-pointer calls (shrinks again after a large history, see StageBuffer)
  uint32_t* bins;     // [kSchedBins]
  int32_t* order;     // [n]
  bool schedule;      // walk the envs longest cycle first (see robot_schedule_*)
  int64_t max_steps;  // robot_max_steps(dt), counted at create
  int period;         // the rollout kernel's service period M, one of kRolloutPeriods (salp_robot_params.h)
};

struct salp_robot_policy : PolicyObject {     // salp_policy_object.h; last_stream: its most recent upload, rollout or noise-step write
  salp_robot_vec* h;         // the handle it is bound to
};

// What a policy of this handle is checked against and made for: obs_dim 6, act_dim 3, and kmax = 3, which the descriptor's
// ranges ask of a snake handle; a NULL handle: zeros.
static PolicyDims policy_dims(const salp_robot_vec* h) {
  return h ? PolicyDims{ROBOT_POLICY_OBS, ROBOT_POLICY_ACT, 3, h->n, h->device} : PolicyDims{};
}

// Below this many envs every wavefront has an execution unit to itself and the launch lasts as long as
// its slowest env whatever the order.  SALP_ROBOT_SCHEDULE=0/1 overrides (tests run both ways).
static const int64_t kScheduleMinEnvs = 32768;

static int launch_robot_step(salp_robot_vec* h, const float* act, float* obs, float* reward, uint8_t* terminated,
                             uint8_t* truncated, float* final_obs, int32_t* inner_steps, hipStream_t st,
                             const RobotHistory* hist = nullptr) {
  const int32_t* order = nullptr;
  if (h->schedule) {
    HIP_TRY(hipMemsetAsync(h->bins, 0, kSchedBins * sizeof(uint32_t), st));
    int rc = launch_1d(robot_schedule_count, h->n, kSchedBlock, st, h->P, act, h->bins);
    if (rc == SALP_OK) rc = launch_1d(robot_schedule_scan, kSchedBins, kSchedBins, st, h->bins);     // one workgroup
    if (rc == SALP_OK) rc = launch_1d(robot_schedule_scatter, h->n, kSchedBlock, st, h->P, act, h->bins, h->order);
    if (rc != SALP_OK) return rc;
    order = h->order;
  }
  if (hist && hist->count > 0)
    return launch_1d(salp_robot_step_record_kernel, h->n, kRBlock, st, h->P, h->S, act, obs, reward, terminated, truncated,
                     final_obs, inner_steps, order, *hist);
  return launch_1d(salp_robot_step_kernel, h->n, kRBlock, st, h->P, h->S, act, obs, reward, terminated, truncated, final_obs,
                   inner_steps, order);
}

// The rollout kernel of the handle's service period, for the action source ACT and the output signature SIG.
template <int ACT, int SIG>
static int launch_robot_rollout(const salp_robot_vec* h, hipStream_t st, const RobotRollout& J) {
  switch (h->period) {
    case 0: return launch_1d(salp_robot_rollout_kernel<ACT, 0, SIG>, h->n, kRBlock, st, h->P, h->S, J);
    case 32: return launch_1d(salp_robot_rollout_kernel<ACT, 32, SIG>, h->n, kRBlock, st, h->P, h->S, J);
    case 128: return launch_1d(salp_robot_rollout_kernel<ACT, 128, SIG>, h->n, kRBlock, st, h->P, h->S, J);
    default: return launch_1d(salp_robot_rollout_kernel<ACT, 512, SIG>, h->n, kRBlock, st, h->P, h->S, J);
  }
}

// salp_robot_vec_rollout (ACT = kActRead, source = the actions), salp_robot_vec_rollout_policy (kActPolicy, source = the
// policy's device block, which is on the device whatever `flags` says) and salp_robot_vec_rollout_policy_sampled
// (kActPolicySampled, the same source; behind the rollout kernel the block's noise step goes on by the horizon, in the
// host-pointer form before the copies out); everything is checked before anything is launched.
template <int ACT>
static int robot_rollout_impl(salp_robot_vec_t* h, const float* source, int32_t horizon, float* obs, float* reward,
                              uint8_t* terminated, uint8_t* truncated, float* final_obs, int32_t* inner_steps, float* act_out,
                              uint32_t flags, void* stream, float* logp_out = nullptr) {
  char why[160];
  if (const int bad = check_rollout_args(h->max_steps, horizon, flags, source != nullptr,
                                         obs || reward || terminated || truncated, why, sizeof(why)))
    return fail(bad, why);
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  RobotRollout J = {};
  J.horizon = horizon; J.max_iters = rollout_max_iters(horizon, h->max_steps, h->period);
  const size_t n = (size_t)h->n, HN = (size_t)horizon * n;
  HostStream s[] = {stream_in(ACT == kActRead ? source : nullptr, HN * 3), stream_out(obs, HN * 6), stream_out(reward, HN),
                    stream_out(terminated, HN), stream_out(truncated, HN), stream_out(final_obs, HN * 6, true),
                    stream_out(inner_steps, HN), stream_out(act_out, HN * 3), stream_out(logp_out, HN)};
  return staged(h->stage, f.st, flags & 1u, s, [&] {
    J.act = ACT == kActRead ? s[0].as<const float>() : source;
    J.obs = s[1].as<float>(); J.reward = s[2].as<float>(); J.terminated = s[3].as<uint8_t>(); J.truncated = s[4].as<uint8_t>();
    J.final_obs = s[5].as<float>(); J.inner_steps = s[6].as<int32_t>(); J.act_out = s[7].as<float>();
    J.logp_out = s[8].as<float>();
    const int rc = launch_robot_rollout<ACT, kSigSteps>(h, f.st, J);
    if (ACT != kActPolicySampled || rc != SALP_OK) return rc;
    return policy_noise_advance(const_cast<float*>(source), horizon, f.st);
  });
}

// salp_robot_vec_evaluate_policy (ACT = kActPolicy) and salp_robot_vec_evaluate_policy_sampled (kActPolicySampled): the
// closed loop of robot_rollout_impl with the summary signature, one record per robot in `rec`, which goes in as well as out
// in the host-pointer form; everything is checked before anything is launched.
template <int ACT>
static int robot_evaluate_impl(salp_robot_vec_t* h, const salp_robot_policy_t* pol, int32_t horizon, void* rec, uint32_t flags,
                               void* stream) {
  if (!h || !pol) return fail(SALP_ERR_INVALID, "handle / policy is NULL");
  char why[160];
  if (const int bad = check_evaluate_args(h->max_steps, horizon, flags, rec, pol->h == h, ACT == kActPolicySampled, pol->gaussian,
                                          why, sizeof(why)))
    return fail(bad, why);
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  RobotRollout J = {};
  J.horizon = horizon; J.max_iters = rollout_max_iters(horizon, h->max_steps, h->period);
  J.eval_flags = flags & ((uint32_t)SALP_ROBOT_EVAL_ACCUMULATE | (uint32_t)SALP_ROBOT_EVAL_FIRST_EPISODE);
  J.act = pol->block;
  HostStream s[] = {stream_out(static_cast<int32_t*>(rec), (size_t)h->n * SALP_REVAL_WORDS, true)};
  const int rc = staged(h->stage, f.st, flags & 1u, s, [&] {
    J.rec = s[0].as<int32_t>();
    const int launched = launch_robot_rollout<ACT, kSigSummary>(h, f.st, J);
    if (ACT != kActPolicySampled || launched != SALP_OK) return launched;
    return policy_noise_advance(pol->block, horizon, f.st);
  });
  if (rc == SALP_OK) pol->last_stream = (hipStream_t)stream;
  return rc;
}

extern "C" {

const char* salp_robot_last_error(void) { return g_err.c_str(); }

int salp_robot_config_default(salp_robot_config_t* c) {
  if (!c) return fail(SALP_ERR_INVALID, "cfg is NULL");
  robot_config_default(c);
  return 0;
}

int salp_robot_vec_create(const salp_robot_config_t* cfg, int64_t n_envs, int device_id, uint64_t seed,
                          int64_t env_index_base, salp_robot_vec_t** out) {
  if (!out) return fail(SALP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  const char* why = "";
  if (const int bad = check_robot_create(cfg, n_envs, env_index_base, &why)) return fail(bad, why);
  int rc = check_device_id(device_id);
  if (rc != SALP_OK) return rc;
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(device_id));
  salp_robot_vec* h = new (std::nothrow) salp_robot_vec();     // value-initialised: every field zero
  if (!h) return fail(SALP_ERR_OOM, "host allocation failed");
  h->cfg = *cfg; h->device = device_id; h->n = n_envs;
  h->stage.shrink = true;
  h->max_steps = robot_max_steps(cfg->dt);
  h->P = make_robot_params(*cfg, n_envs, seed, env_index_base);
  h->schedule = n_envs >= kScheduleMinEnvs;
  if (const char* ev = getenv("SALP_ROBOT_SCHEDULE")) h->schedule = ev[0] == '1';
  if (n_envs > INT32_MAX) h->schedule = false;
  h->period = kRolloutPeriod;     // SALP_ROBOT_ROLLOUT_M=0/32/128/512 overrides (profiles/robot_rollout_perf.py measures them all)
  if (const char* ev = getenv("SALP_ROBOT_ROLLOUT_M"))
    for (const int m : kRolloutPeriods)
      if (atoi(ev) == m) h->period = m;
  const size_t bytes = (size_t)SALP_R_COUNT * (size_t)h->P.pitch * sizeof(double);
  hipError_t e = hipMalloc((void**)&h->S.f, bytes);
  if (e == hipSuccess) e = hipMemset(h->S.f, 0, bytes);
  if (e == hipSuccess && h->schedule) e = hipMalloc((void**)&h->bins, kSchedBins * sizeof(uint32_t));
  if (e == hipSuccess && h->schedule) e = hipMalloc((void**)&h->order, (size_t)n_envs * sizeof(int32_t));
  if (e != hipSuccess) rc = fail(SALP_ERR_OOM, std::string("state allocation: ") + hipGetErrorString(e));
  if (rc == 0) rc = salp_robot_vec_reset(h, nullptr, nullptr, 1u, nullptr);   // train_robot.py:16 angles (0, 0) are the zeroed rows
  if (rc == 0 && hipDeviceSynchronize() != hipSuccess) rc = fail(SALP_ERR_HIP, "initial reset failed");
  if (rc != 0) { const std::string m = g_err; salp_robot_vec_destroy(h); g_err = m; return rc; }   // the one failure path
  *out = h;
  return 0;
}

void salp_robot_vec_destroy(salp_robot_vec_t* h) {
  if (!h) return;
  DeviceScope dev_scope;
  (void)dev_scope.enter(h->device);
  if (h->S.f) (void)hipFree(h->S.f);
  if (h->bins) (void)hipFree(h->bins);
  if (h->order) (void)hipFree(h->order);
  delete h;     // the staging block goes with it
}

int64_t salp_robot_vec_num_envs(const salp_robot_vec_t* h) { return h ? h->n : 0; }

int salp_robot_vec_reset(salp_robot_vec_t* h, const uint8_t* mask, float* obs, uint32_t flags, void* stream) {
  if (!h) return fail(SALP_ERR_INVALID, "handle is NULL");
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  HostStream s[] = {stream_in(mask, (size_t)h->n), stream_out(obs, (size_t)h->n * 6)};
  return staged(h->stage, f.st, flags & 1u, s, [&] {
    return launch_1d(salp_robot_reset_kernel, h->n, kRBlock, f.st, h->P, h->S, s[0].as<const uint8_t>(), s[1].as<float>(), 1);
  });
}

// salp_robot_vec_step (H == NULL) and salp_robot_vec_step_history (H: the caller's range and pointers, count > 0);
// the arguments have been checked.
static int robot_step_impl(salp_robot_vec_t* h, const float* act, float* obs, float* reward, uint8_t* terminated,
                           uint8_t* truncated, float* final_obs, int32_t* inner_steps, const RobotHistory* H, uint32_t flags,
                           void* stream) {
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  hipStream_t st = f.st;
  // The two forms are kept apart here: with a history the host-pointer form is more than copies around the launch (a
  // scratch piece for the samples, a second copy once the lengths are known), which staged() does not take on.
  if (flags & 1u) return launch_robot_step(h, act, obs, reward, terminated, truncated, final_obs, inner_steps, st, H);
  // host pointers.  final_obs goes in as well as out: only the rows of ended episodes are written.  The history stays on
  // the device until the lengths are known (they are fetched even when the caller does not want them): it goes back as
  // `count` rows of the longest record of this call, one 2-D copy; nothing is copied in, so in rows with a shorter
  // record the samples past history_len are overwritten with unspecified values.
  const size_t n = (size_t)h->n, rows = H ? (size_t)H->count : 0;
  const size_t row = H ? (size_t)H->capacity * SALP_H_COUNT * sizeof(float) : 0;
  std::vector<int32_t> len(rows);
  HostStream s[] = {stream_in(act, n * 3), stream_out(obs, n * 6), stream_out(final_obs, n * 6, true), stream_out(reward, n),
                    stream_out(terminated, n), stream_out(truncated, n), stream_out(inner_steps, n),
                    stream_out(H ? len.data() : nullptr, rows), stream_scratch(rows * row)};
  const int rc = staged(h->stage, st, false, s, [&] {
    RobotHistory D;
    if (H) { D = *H; D.len = s[7].as<int32_t>(); D.hist = s[8].as<float>(); }
    return launch_robot_step(h, s[0].as<const float>(), s[1].as<float>(), s[3].as<float>(), s[4].as<uint8_t>(), s[5].as<uint8_t>(),
                             s[2].as<float>(), s[6].as<int32_t>(), st, H ? &D : nullptr);
  });
  if (rc != 0 || !H) return rc;
  int32_t longest = 0;
  for (int32_t v : len) longest = v > longest ? v : longest;
  HIP_TRY(hipMemcpy2DAsync(H->hist, row, s[8].dev, row, (size_t)longest * SALP_H_COUNT * sizeof(float), rows,
                           hipMemcpyDeviceToHost, st));
  if (H->len) memcpy(H->len, len.data(), rows * sizeof(int32_t));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

int salp_robot_vec_step(salp_robot_vec_t* h, const float* act, float* obs, float* reward, uint8_t* terminated,
                        uint8_t* truncated, float* final_obs, int32_t* inner_steps, uint32_t flags, void* stream) {
  if (!h || !act) return fail(SALP_ERR_INVALID, "handle / act is NULL");
  return robot_step_impl(h, act, obs, reward, terminated, truncated, final_obs, inner_steps, nullptr, flags, stream);
}

int32_t salp_robot_vec_history_capacity(const salp_robot_vec_t* h, int32_t stride) {
  if (!h || stride < 1) return -1;
  return (int32_t)history_capacity(h->max_steps, stride);
}

int salp_robot_vec_step_history(salp_robot_vec_t* h, const float* act, float* obs, float* reward, uint8_t* terminated,
                                uint8_t* truncated, float* final_obs, int32_t* inner_steps, int64_t hist_begin,
                                int64_t hist_count, int32_t stride, int32_t capacity, float* history,
                                int32_t* history_len, uint32_t flags, void* stream) {
  if (!h || !act) return fail(SALP_ERR_INVALID, "handle / act is NULL");
  char why[160];
  bool plain_step;
  if (const int bad = check_history_args(h->n, h->max_steps, hist_begin, hist_count, stride, capacity, history, flags,
                                         &plain_step, why, sizeof(why)))
    return fail(bad, why);
  RobotHistory H;
  H.hist = history; H.len = history_len; H.begin = hist_begin; H.count = hist_count; H.stride = stride; H.capacity = capacity;
  return robot_step_impl(h, act, obs, reward, terminated, truncated, final_obs, inner_steps, plain_step ? nullptr : &H, flags,
                         stream);
}

int salp_robot_vec_trajectory(salp_robot_vec_t* h, const double* params, const double* actions, int32_t cycles,
                              const double* expected, double* states, double* metrics, int32_t* inner_steps,
                              uint32_t flags, void* stream) {
  if (!h || !actions) return fail(SALP_ERR_INVALID, "handle / actions is NULL");
  char why[160];
  if (const int bad = check_trajectory_args(h->max_steps, cycles, flags, expected != nullptr, metrics != nullptr, why, sizeof(why)))
    return fail(bad, why);
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  const bool per_robot = (flags & SALP_ROBOT_PER_ROBOT_ACTIONS) != 0;
  RobotTrajectory J;
  J.cycles = cycles; J.per_robot = per_robot ? 1 : 0;
  const size_t n = (size_t)h->n, T = (size_t)cycles;
  HostStream s[] = {stream_in(params, (size_t)SALP_RP_COUNT * n), stream_in(actions, T * (per_robot ? n : 1) * 3),
                    stream_in(expected, T * 6), stream_out(states, T * n * 6), stream_out(metrics, n * SALP_RM_COUNT),
                    stream_out(inner_steps, T * n)};
  return staged(h->stage, f.st, flags & 1u, s, [&] {
    J.params = s[0].as<const double>(); J.actions = s[1].as<const double>(); J.expected = s[2].as<const double>();
    J.states = s[3].as<double>(); J.metrics = s[4].as<double>(); J.inner_steps = s[5].as<int32_t>();
    return launch_1d(salp_robot_trajectory_kernel, h->n, kRBlock, f.st, h->P, J);
  });
}

int salp_robot_vec_rollout(salp_robot_vec_t* h, const float* act, int32_t horizon, float* obs, float* reward,
                           uint8_t* terminated, uint8_t* truncated, float* final_obs, int32_t* inner_steps,
                           uint32_t flags, void* stream) {
  if (!h) return fail(SALP_ERR_INVALID, "handle is NULL");
  return robot_rollout_impl<kActRead>(h, act, horizon, obs, reward, terminated, truncated, final_obs, inner_steps, nullptr, flags,
                                      stream);
}

// The policy object's calls: salp_policy_object.h.
int salp_robot_policy_words(const salp_robot_vec_t* h, const salp_policy_desc_t* desc) { return policy_words(policy_dims(h), desc, false); }
int salp_robot_policy_words_gaussian(const salp_robot_vec_t* h, const salp_policy_desc_t* desc) { return policy_words(policy_dims(h), desc, true); }

void salp_robot_policy_destroy(salp_robot_policy_t* pol) {
  if (pol) policy_free(pol, nullptr);     // its uploads and the rollouts that read the block are all on its own last_stream
}

// salp_robot_policy_create (gaussian = false) and salp_robot_policy_create_gaussian
static int robot_policy_create_impl(salp_robot_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags,
                                    void* stream, salp_robot_policy_t** out, bool gaussian) {
  // of `flags`, bit 0 (device pointers) is the known one: any other is refused, behind out, the descriptor and weights
  const int rc = policy_create(policy_dims(h), desc, weights, flags, 1u, stream, gaussian, out);
  if (rc == SALP_OK) (*out)->h = h;
  return rc;
}

int salp_robot_policy_create(salp_robot_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags,
                             void* stream, salp_robot_policy_t** out) {
  return robot_policy_create_impl(h, desc, weights, flags, stream, out, false);
}

int salp_robot_policy_create_gaussian(salp_robot_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags,
                                      void* stream, salp_robot_policy_t** out) {
  return robot_policy_create_impl(h, desc, weights, flags, stream, out, true);
}

int salp_robot_policy_set_noise_step(salp_robot_policy_t* pol, uint64_t n, void* stream) {
  if (!pol) return fail(SALP_ERR_INVALID, "policy is NULL");
  return policy_set_noise_step(*pol, n, stream);
}

int salp_robot_policy_noise_step(salp_robot_policy_t* pol, uint64_t* n) {
  if (!pol || !n) return fail(SALP_ERR_INVALID, "policy/n is NULL");
  return policy_noise_step(*pol, n);
}

int salp_robot_policy_update(salp_robot_policy_t* pol, const float* weights, uint32_t flags, void* stream) {
  if (!pol || !weights) return fail(SALP_ERR_INVALID, "policy/weights is NULL");
  if (flags & ~1u) return fail(SALP_ERR_INVALID, "unknown flag bits");
  return policy_update(*pol, weights, (flags & 1u) != 0, stream);
}

int salp_robot_vec_rollout_policy(salp_robot_vec_t* h, const salp_robot_policy_t* pol, int32_t horizon, float* obs,
                                  float* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs,
                                  int32_t* inner_steps, float* act_out, uint32_t flags, void* stream) {
  if (!h || !pol) return fail(SALP_ERR_INVALID, "handle / policy is NULL");
  if (pol->h != h) return fail(SALP_ERR_INVALID, "the policy belongs to another handle");
  // (the descriptor passed check_policy_desc at create with this handle: one policy per wavefront holds)
  const int rc = robot_rollout_impl<kActPolicy>(h, pol->block, horizon, obs, reward, terminated, truncated, final_obs, inner_steps,
                                                act_out, flags, stream);
  if (rc == SALP_OK) pol->last_stream = (hipStream_t)stream;
  return rc;
}

// The policy arrives const (the signature mirrors the deterministic twin's), yet the call advances its noise word in device
// memory and writes its last_stream (`mutable`): include/salp_robot_sampled.h says so.
int salp_robot_vec_rollout_policy_sampled(salp_robot_vec_t* h, const salp_robot_policy_t* pol, int32_t horizon, float* obs,
                                          float* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs,
                                          int32_t* inner_steps, float* act_out, float* logp_out, uint32_t flags, void* stream) {
  if (!h || !pol) return fail(SALP_ERR_INVALID, "handle / policy is NULL");
  if (pol->h != h) return fail(SALP_ERR_INVALID, "the policy belongs to another handle");
  if (!pol->gaussian) return fail(SALP_ERR_INVALID, "sampling needs a Gaussian policy (salp_robot_policy_create_gaussian)");
  const int rc = robot_rollout_impl<kActPolicySampled>(h, pol->block, horizon, obs, reward, terminated, truncated, final_obs,
                                                       inner_steps, act_out, flags, stream, logp_out);
  if (rc == SALP_OK) pol->last_stream = (hipStream_t)stream;
  return rc;
}

int salp_robot_vec_evaluate_policy(salp_robot_vec_t* h, const salp_robot_policy_t* pol, int32_t horizon, void* rec, uint32_t flags,
                                   void* stream) {
  return robot_evaluate_impl<kActPolicy>(h, pol, horizon, rec, flags, stream);
}

// (the policy arrives const and its noise word is advanced all the same, as in salp_robot_vec_rollout_policy_sampled)
int salp_robot_vec_evaluate_policy_sampled(salp_robot_vec_t* h, const salp_robot_policy_t* pol, int32_t horizon, void* rec,
                                           uint32_t flags, void* stream) {
  return robot_evaluate_impl<kActPolicySampled>(h, pol, horizon, rec, flags, stream);
}

int salp_robot_vec_get_state(salp_robot_vec_t* h, double* state, uint32_t flags, void* stream) {
  if (!h || !state) return fail(SALP_ERR_INVALID, "handle / state is NULL");
  CallFrame f;
  if (const int rc = f.enter(h, stream)) return rc;
  hipStream_t st = f.st;
  // rows are [pitch] on the device and [n] in the snapshot
  HIP_TRY(hipMemcpy2DAsync(state, (size_t)h->n * sizeof(double), h->S.f, (size_t)h->P.pitch * sizeof(double),
                            (size_t)h->n * sizeof(double), SALP_R_COUNT,
                            (flags & 1u) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  if (!(flags & 1u)) HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

// Test support (salp_fp64_math.h): one of the fp64 primitives over host arrays, staged like the other host-pointer calls.
int salp_robot_math_probe(int device_id, int function, const double* in, double* out, int64_t n, int32_t steps) {
  if (!in || !out) return fail(SALP_ERR_INVALID, "in / out is NULL");
  if (n < 1 || n > ((int64_t)1 << 24)) return fail(SALP_ERR_INVALID, "n must be in [1, 2^24]");
  size_t rows_in = 1, rows_out = 2;
  switch (function) {
    case SALP_MATH_SINCOS_SMALL: case SALP_MATH_SINCOS_EULER: break;
    case SALP_MATH_ROTATE: rows_in = 3; break;
    case SALP_MATH_CHAIN:
      if (steps < 0 || steps > 65536) return fail(SALP_ERR_INVALID, "steps must be in [0, 65536]");
      rows_in = 1 + (size_t)steps; rows_out = 3;
      break;
    case SALP_MATH_RCP_NR: case SALP_MATH_SQRT_NR: rows_out = 1; break;
    default: return fail(SALP_ERR_INVALID, "unknown function code");
  }
  if (rows_in * (size_t)n * sizeof(double) > ((size_t)1 << 31)) return fail(SALP_ERR_INVALID, "input larger than 2 GiB");
  const int rc = check_device_id(device_id);
  if (rc != SALP_OK) return rc;
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(device_id));
  StageBuffer stage;     // the call's own, released on return
  HostStream s[] = {stream_in(in, rows_in * (size_t)n), stream_out(out, rows_out * (size_t)n)};
  return staged(stage, nullptr, false, s, [&] {
    return launch_1d(salp_robot_math_probe_kernel, n, kRBlock, nullptr, function, s[0].as<const double>(), s[1].as<double>(), n, steps);
  });
}

}  // extern "C"
