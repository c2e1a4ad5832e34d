/*
 * salp_robot_sampled.h — C ABI of the stochastic (tanh-Gaussian) form of the in-kernel policy of the batched HEAD simulator:
 * the multi-cycle closed-loop rollout of salp_robot_rollout.h with every action SAMPLED in the kernel and its
 * log-probability returned.  The handle is the salp_robot_vec_t of salp_robot.h, the policy object the salp_robot_policy_t
 * of salp_robot_rollout.h; the policy descriptor salp_policy_desc_t, the status codes and SALP_DEVICE_PTRS are those of
 * salp_vec.h.  The functions are part of the same library.  Every number below comes from salp_vec.h ("Randomness",
 * "Sampled actions"), with three action components in place of one or two.
 *
 * Noise.  block_k(env, n) = Philox4x32-10(counter = (env_lo, env_hi, n, 3 + k), key = the handle's (seed_lo, seed_hi)).
 *   - components 0 and 1 take the words (w0, w1) and (w2, w3) of block_0: exactly the definition of salp_vec.h;
 *   - component 2 takes (w0, w1) of block_1, that is, the fourth counter word 4, which nothing else uses (salp_vec.h uses
 *     0..3, the robot's reset draw 16);
 *   - env is the GLOBAL env index (env_index_base + local index);
 *   - n is the low 32 bits of n0 + t: n0 the policy's 64-bit noise step read at kernel entry, t that env's own step index
 *     within the call.  The lanes of a launch reach their steps at different times; the draw depends on (env, t) only;
 *   - one standard normal draw per component from its two words (wa, wb), fp32 (Box-Muller, unchanged):
 *       u1 = ((wa >> 8) + 1) * 2^-24  in (0, 1]     u2 = (wb >> 8) * 2^-24  in [0, 1)
 *       z  = sqrtf(-2 * logf(u1)) * cospif(2 * u2)
 *   - the env's own draw counter (state row SALP_R_RNG) is not consumed: the simulator's trajectory stays a function of the
 *     actions alone.
 *
 * Sampled action and log-probability.  Per action component j = 0, 1, 2, fp32, in one fixed order (z_j: the draw above):
 *   mu = mean head (the deterministic arithmetic of salp_robot_rollout.h);  ls = the log-std head in the same fmaf order
 *   (every unit starts from its bias and adds its inputs in index order with one fmaf each), then
 *   ls = fminf(fmaxf(ls, -20), 2);  sd = expf(ls);  u = fmaf(sd, z, mu);  a = tanhf(u) * scale + shift   (two roundings)
 *   m = -2 * u;  sp = fmaxf(m, 0) + log1pf(expf(-fabsf(m)));  c = (log 2 - u) - sp
 *   g = -0.5 * (z * z);  g = g - ls;  g = g - 0.5 log(2 pi);  g = g - 2 * c;      logp = 0 + g_0 + g_1 + g_2, in index order
 * — sac.Actor.forward's value with (u - mu) / std taken as z.  Every operation above is one fp32 rounding (no contraction).
 *
 * Gaussian policy (salp_robot_policy_words_gaussian, salp_robot_policy_create_gaussian).  Weights of ONE policy, float32:
 * the hidden layers as in salp_robot_rollout.h; then the mean head W_mu[3][in], b_mu[3]; then the log-std head W_ls[3][in],
 * b_ls[3]; then scale[3], shift[3].  out_activation must be SALP_POLICY_OUT_TANH; the other ranges and the n_policies rule
 * are those of salp_robot_policy_create.  The result is an ordinary salp_robot_policy_t: salp_robot_policy_update takes
 * the Gaussian layout for it, salp_robot_policy_destroy releases it, and salp_robot_vec_rollout_policy on it runs its MEAN
 * — every output equals, bit for bit, that of the plain policy built from the same body and mean head.
 *
 * Noise step (salp_robot_policy_set_noise_step, salp_robot_policy_noise_step).  A 64-bit device word owned by the policy
 * object, 0 after create.  set: stream-ordered (a one-thread kernel on `stream`).  get: waits for the stream of the
 * policy's most recent create / update / set / rollout call, then reads the word with a blocking copy — so it must not be
 * called while a stream is capturing.  Ordering is stream ordering and nothing else.  SALP_ERR_INVALID for a policy that is
 * not Gaussian (and for NULL arguments).
 *
 * salp_robot_vec_rollout_policy_sampled.  salp_robot_vec_rollout_policy with the sampled actions: which observation each
 * action sees, n_policies > 1, autoreset, state write-back, SALP_DEVICE_PTRS, host staging, the nullable outputs and the
 * "at least one of obs, reward, terminated, truncated" rule are the deterministic twin's.  act_out (nullable) float
 * [H][n][3] receives the actions taken, logp_out (nullable) float [H][n] their log-probabilities.  A one-thread kernel
 * enqueued behind the rollout adds `horizon` to the policy's noise step: stream-ordered and capturable, so a replayed
 * hipGraph draws fresh noise (should that last launch itself fail, the call returns the HIP error with the envs stepped
 * and the noise step not advanced: set it before sampling on).  The policy arrives const and its noise word is advanced
 * all the same: a salp_robot_policy_t is not thread-safe, like the handle it is bound to.
 * SALP_ERR_INVALID, with nothing launched and the state and the noise step untouched, for everything
 * salp_robot_vec_rollout_policy refuses and for a policy that is not Gaussian.
 */
#ifndef SALP_ROBOT_SAMPLED_H
#define SALP_ROBOT_SAMPLED_H
#include <stdint.h>
#include "salp_vec.h"             /* salp_policy_desc_t, the status codes, SALP_DEVICE_PTRS */
#include "salp_robot.h"           /* salp_robot_vec_t */
#include "salp_robot_rollout.h"   /* salp_robot_policy_t */
#ifdef __cplusplus
extern "C" {
#endif

/* float32 words of one Gaussian policy in the public layout, or the negative status */
int salp_robot_policy_words_gaussian(const salp_robot_vec_t* h, const salp_policy_desc_t* desc);
int salp_robot_policy_create_gaussian(salp_robot_vec_t* h, const salp_policy_desc_t* desc, const float* weights,
                                      uint32_t flags, void* stream, salp_robot_policy_t** out);
int salp_robot_policy_set_noise_step(salp_robot_policy_t* pol, uint64_t n, void* stream);
int salp_robot_policy_noise_step(salp_robot_policy_t* pol, uint64_t* n);

/* the closed-loop rollout with sampled actions; act_out (nullable) float [H][n][3], logp_out (nullable) float [H][n] */
int salp_robot_vec_rollout_policy_sampled(salp_robot_vec_t* h, const salp_robot_policy_t* pol, int32_t horizon, float* obs,
                                          float* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs,
                                          int32_t* inner_steps, float* act_out, float* logp_out, uint32_t flags,
                                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
