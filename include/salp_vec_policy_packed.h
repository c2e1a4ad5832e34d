/*
 * salp_vec_policy_packed.h — C ABI of the closed-loop rollouts that return packed transition records: the in-kernel policy
 * of salp_vec_rollout_policy (and its sampling form) as the action source, the record of salp_vec_rollout_packed as the one
 * output stream.  The handle, the policy object, the record layout, the status codes and the flags are those of salp_vec.h;
 * the functions are part of the same library.
 *
 *   salp_vec_rollout_policy_packed           `horizon` x (a = policy(obs); record = step(a)) in one launch
 *   salp_vec_rollout_policy_packed_sampled   the same loop with the sampled actions of a Gaussian policy
 *
 * Why: salp_vec_rollout_policy returns obs, reward, terminated and truncated only — a closed loop had no terminal observation
 * and no info, so a replay buffer fed from it lost the transitions SAC must bootstrap through (every truncated step: after the
 * same-step autoreset obs[t] is the next episode's first row), and a demo recorder (the reference's
 * scripts/collection/collect_agent_demos.py keeps obs, action, next obs, done and info per step) could not use it.
 *
 * Nothing new is defined: the semantics are the union of the two parents in salp_vec.h.
 *   From salp_vec_rollout_policy / salp_vec_rollout_policy_sampled ("Policy", "Gaussian policy", "Sampled actions"): which
 *   observation each action sees — the action of step 0 is the policy applied to the env's current observation, formed with
 *   the bits of the step that left the state (a rollout cut into several calls takes the actions of one call), the action of
 *   step t + 1 is the policy applied to the observation words of record t (after a same-step autoreset: the first row of the
 *   new episode); the policy assignment for P > 1; the noise blocks, and the advance of the policy's noise step by `horizon`
 *   behind the launches (sampled form only; should that last one-thread launch fail, the call returns the HIP error with the
 *   envs stepped and the noise step not advanced); act_out (may be NULL) float [horizon][n_envs][act_dim], the actions taken;
 *   logp_out (sampled form only, may be NULL) float [horizon][n_envs]; the state write-back, the global step, the statistics,
 *   the split launch for ragged n_envs; with SALP_DEVICE_PTRS the call only launches kernels on `stream` (capturable into a
 *   hipGraph; salp_policy_update may sit between two replays).
 *   From salp_vec_rollout_packed ("Packed transition record"): rec is [horizon][n_envs][salp_vec_record_width(h, flags)] words
 *   in that layout; reward, flags word and the two info counters hold the values of the step's own episode (before the
 *   autoreset), byte 3 of the flags word is zero; with SALP_REC_FINAL_OBS every record has obs_dim more words, written only in
 *   the rows of envs that finished in that step (the others keep what the caller put there); a device block must be 16-byte
 *   aligned.  With host pointers the call is synchronous and rec goes in as well as out when SALP_REC_FINAL_OBS is set.
 * The log-probability is not part of the record: it leaves through logp_out.  A record block of these calls equals, word for
 * word, the block salp_vec_rollout_packed writes from the same state on the actions in act_out, and its observation, reward and
 * flag words equal the streams of salp_vec_rollout_policy(_sampled) from the same state (and noise step).
 *
 * flags: SALP_DEVICE_PTRS and / or SALP_REC_FINAL_OBS.
 * SALP_ERR_INVALID, with nothing launched and the handle and the noise step unchanged: a NULL handle, policy or rec;
 * horizon < 1; any other flag bit; a device rec that is not 16-byte aligned; a policy of another handle or of other dimensions;
 * a P that n_envs does not allow; a handle with max_observed_food != 3 (no policy can be created for one); for the sampled
 * form, a policy that is not Gaussian.  (A Gaussian policy given to the deterministic form runs its mean.)
 * salp_vec_last_launch reports signature 3 with action source 2 (deterministic) or 3 (sampled), in both halves of a split
 * launch.
 */
#ifndef SALP_VEC_POLICY_PACKED_H
#define SALP_VEC_POLICY_PACKED_H
#include <stdint.h>
#include "salp_vec.h"     /* salp_vec_t, salp_policy_t, the record layout, the status codes, SALP_DEVICE_PTRS, SALP_REC_FINAL_OBS */
#ifdef __cplusplus
extern "C" {
#endif

/* rec float / int32 words [horizon][n_envs][width]; act_out (nullable) float [horizon][n_envs][act_dim] */
int salp_vec_rollout_policy_packed(salp_vec_t* h, const salp_policy_t* pol, int32_t horizon, float* rec, float* act_out,
                                   uint32_t flags, void* stream);
/* the same with sampled actions; logp_out (nullable) float [horizon][n_envs] */
int salp_vec_rollout_policy_packed_sampled(salp_vec_t* h, const salp_policy_t* pol, int32_t horizon, float* rec, float* act_out,
                                           float* logp_out, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SALP_VEC_POLICY_PACKED_H */
