// salp_policy_object.h — the in-kernel policy as an object of the C ABI: the three device allocations behind a
// salp_policy_t (salp_vec.hip) and a salp_robot_policy_t (salp_robot.hip) and their whole life: descriptor check, create,
// upload, update, noise step, free.  Host only, internal linkage like salp_host.h, and included after it: each of the
// two translation units writes its own error string.  The functions take the handle's dimensions (PolicyDims), not a
// handle; what the two libraries do differently stays in their ABI files (which flag bits create / update refuse, whose
// streams destroy waits for, who records last_stream after a rollout).  What is decided before a GPU is touched —
// ranges, block map, header, byte counts — is salp_policy.h; the kernels behind upload and noise step are reached
// through salp_policy_upload.h.
#ifndef SALP_POLICY_OBJECT_H
#define SALP_POLICY_OBJECT_H

#include <new>
#include <string>
#include <vector>

#include "salp_host.h"
#include "salp_policy.h"
#include "salp_policy_wide.h"
#include "salp_policy_upload.h"

namespace {

// What a policy needs to know of the handle it is bound to.  A NULL handle's dimensions are all zero.
struct PolicyDims {
  int obs_dim, act_dim, kmax;
  int64_t n;                 // the handle's env count (fixes env -> policy)
  int device;
  int food_slots;            // the snake handle's kernel class (1: the one-food kernels); the wide scheme asks for it
};

// The fields of both policy structs; each adds the back-pointer to its handle (`h`).
struct PolicyObject {
  salp_policy_desc_t d;
  int device, obs_dim, act_dim;
  int64_t n;
  int words;                 // public words of one policy
  int stride;                // words of one policy in the device block (salp_policy.h)
  float* block;              // device: header + P policies, what the kernel reads
  float* pub;                // device: staging of the public layout [P][words] (host-pointer create / update)
  int32_t* map;              // device: word k of a policy in the block <- public word map[k] (-1: zero)
  int gaussian;              // *_policy_create_gaussian: a log-std head behind the mean head, a noise step in the header
  int wide;                  // salp_policy_create_wide: the block has the layout of salp_policy_wide.h and runs its kernels
  mutable hipStream_t last_stream;   // the stream of the most recent create / update / noise-step write, and of whatever else the ABI file records
};

// The descriptor's ranges for a handle of these dimensions (salp_policy.h).  On success *words (nullable) = public words
// of one policy.  A NULL handle (n == 0) and a NULL descriptor get one refusal, one text.
int check_policy_dims(const PolicyDims& dims, const salp_policy_desc_t* d, bool gaussian, int* words, bool wide = false) {
  const char* why = "";
  const int rc = wide ? salp::check_policy_desc_wide(dims.obs_dim, dims.act_dim, dims.kmax, dims.food_slots, dims.n, dims.n ? d : nullptr, gaussian, words, &why)
                      : salp::check_policy_desc(dims.obs_dim, dims.act_dim, dims.kmax, dims.n, dims.n ? d : nullptr, gaussian, words, &why);
  return rc == SALP_OK ? rc : fail(rc, why);
}

// *_policy_words and *_policy_words_gaussian
int policy_words(const PolicyDims& dims, const salp_policy_desc_t* d, bool gaussian, bool wide = false) {
  int words = 0;
  const int rc = check_policy_dims(dims, d, gaussian, &words, wide);
  return rc != SALP_OK ? rc : words;
}

// *_policy_destroy: waits for the policy's own stream and for `readers` (nullable: a stream on which launches that read
// the block were recorded elsewhere) — hipFree does not wait for kernels on non-blocking streams.
template <class Policy>
void policy_free(Policy* pol, const hipStream_t* readers) {
  DeviceScope dev_scope;
  (void)dev_scope.enter(pol->device);
  (void)hipStreamSynchronize(pol->last_stream);
  if (readers) (void)hipStreamSynchronize(*readers);
  if (pol->block) (void)hipFree(pol->block);
  if (pol->pub) (void)hipFree(pol->pub);
  if (pol->map) (void)hipFree(pol->map);
  delete pol;
}

// *_policy_update, and the first upload of create: new weights into the block on `stream`; `pol` and `weights` are not NULL
int policy_update(const PolicyObject& pol, const float* weights, bool device_ptrs, void* stream) {
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(pol.device));
  pol.last_stream = (hipStream_t)stream;
  const salp::PolicyBlock b = {pol.block, pol.pub, pol.map, pol.d.n_policies, pol.words, pol.stride};
  HIP_TRY(salp::policy_block_upload(b, weights, device_ptrs, pol.last_stream));
  return SALP_OK;
}

// *_policy_create and *_policy_create_gaussian: checks in the order out, descriptor, weights, flags (`known_flags`: a bit
// outside is refused; bit 0 says device pointers), then the block map, the three allocations, map and header, the first
// upload.  On success **out is zero but for the shared fields: the caller sets its back-pointer.  `wide`: the ranges, the
// block map and the header of salp_policy_wide.h instead.
template <class Policy>
int policy_create(const PolicyDims& dims, const salp_policy_desc_t* desc, const float* weights, uint32_t flags, uint32_t known_flags,
                  void* stream, bool gaussian, Policy** out, bool wide = false) {
  if (!out) return fail(SALP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  int words = 0;
  int rc = check_policy_dims(dims, desc, gaussian, &words, wide);
  if (rc != SALP_OK) return rc;
  if (!weights) return fail(SALP_ERR_INVALID, "weights is NULL");
  if (flags & ~known_flags) return fail(SALP_ERR_INVALID, "unknown flag bits");
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(dims.device));
  Policy* pol = new (std::nothrow) Policy();     // value-initialised: every field zero
  if (!pol) return fail(SALP_ERR_OOM, "host allocation failed");
  pol->d = *desc; pol->device = dims.device; pol->obs_dim = dims.obs_dim; pol->act_dim = dims.act_dim; pol->n = dims.n;
  pol->words = words; pol->gaussian = gaussian ? 1 : 0; pol->wide = wide ? 1 : 0;
  std::vector<int32_t> map;     // word k of a policy in the device block <- public word map[k]: salp_policy.h
  pol->stride = wide ? salp::policy_block_map_wide(dims.act_dim, *desc, gaussian, map)
                     : salp::policy_block_map(dims.obs_dim, dims.act_dim, *desc, gaussian, map);
  const salp::PolicyBytes bytes = salp::policy_bytes(*desc, words, pol->stride);
  hipError_t e = hipMalloc((void**)&pol->block, bytes.block);
  if (e == hipSuccess) e = hipMalloc((void**)&pol->pub, bytes.pub);
  if (e == hipSuccess) e = hipMalloc((void**)&pol->map, bytes.map);
  if (e == hipSuccess) e = hipMemcpy(pol->map, map.data(), bytes.map, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    int32_t hd[salp::PH_WORDS];
    if (wide) salp::policy_header_wide(*desc, pol->stride, dims.n, gaussian, hd);
    else salp::policy_header(*desc, pol->stride, dims.n, gaussian, hd);
    e = hipMemcpy(pol->block, hd, sizeof(hd), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess)
    rc = fail(e == hipErrorOutOfMemory ? SALP_ERR_OOM : SALP_ERR_HIP, std::string("hipMalloc/hipMemcpy(policy): ") + hipGetErrorString(e));
  else
    rc = policy_update(*pol, weights, (flags & 1u) != 0, stream);
  if (rc != SALP_OK) { const std::string m = g_err; policy_free(pol, nullptr); g_err = m; return rc; }   // the one failure path
  *out = pol;
  return SALP_OK;
}

// The noise step of a block goes on by the horizon of a sampled call, on the device, behind the call's launches on `st`.
int policy_noise_advance(float* block, int32_t horizon, hipStream_t st) {
  HIP_TRY(salp::policy_noise_write(block, (uint64_t)horizon, false, st));
  return SALP_OK;
}

// *_policy_set_noise_step; `pol` is not NULL
int policy_set_noise_step(const PolicyObject& pol, uint64_t n, void* stream) {
  if (!pol.gaussian) return fail(SALP_ERR_INVALID, "the policy is not Gaussian: it has no noise step");
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(pol.device));
  pol.last_stream = (hipStream_t)stream;
  HIP_TRY(salp::policy_noise_write(pol.block, n, true, (hipStream_t)stream));
  return SALP_OK;
}

// *_policy_noise_step; `pol` and `n` are not NULL.  Waits for the policy's last stream.
int policy_noise_step(const PolicyObject& pol, uint64_t* n) {
  if (!pol.gaussian) return fail(SALP_ERR_INVALID, "the policy is not Gaussian: it has no noise step");
  DeviceScope dev_scope;
  HIP_TRY(dev_scope.enter(pol.device));
  HIP_TRY(hipStreamSynchronize(pol.last_stream));
  uint32_t w[2] = {0u, 0u};
  HIP_TRY(hipMemcpy(w, reinterpret_cast<const uint32_t*>(pol.block) + salp::PH_NOISE, sizeof(w), hipMemcpyDeviceToHost));
  *n = ((uint64_t)w[1] << 32) | w[0];
  return SALP_OK;
}

}  // namespace

#endif  // SALP_POLICY_OBJECT_H
