/*
 * salp_robot_rollout.h — C ABI of the multi-cycle rollouts of the batched HEAD simulator (salp_robot.h, SURVEY.md
 * §8f-4) and of the small MLP policy that can run inside them.  The handle is the salp_robot_vec_t of salp_robot.h; the
 * policy descriptor salp_policy_desc_t, the status codes and SALP_DEVICE_PTRS are those of salp_vec.h.  The functions are
 * part of the same library.
 *
 *   salp_robot_vec_rollout         `horizon` x SalpRobotEnv.step (salp_robot_env.py:139-201) on recorded actions
 *   salp_robot_policy_*            a deterministic 6 -> 3 MLP policy on the device (model.predict(obs, deterministic=True))
 *   salp_robot_vec_rollout_policy  the closed loop predict -> step, `horizon` times, in one launch
 *
 * Rollouts (salp_robot_vec_rollout, salp_robot_vec_rollout_policy).  `horizon` env steps — `horizon` breathing cycles per
 * robot — in ONE kernel launch, env i on lane i (the cycle-length schedule of salp_robot_vec_step is not used).  A lane
 * begins its next cycle when its own cycle has ended instead of waiting for the slowest env of the launch, so a closed
 * loop needs no host round trip per cycle.  Both calls:
 *   - outputs are time-major: obs float [H][n][6], reward float [H][n], terminated / truncated uint8 [H][n], final_obs
 *     float [H][n][6], inner_steps int32 [H][n].  Every output pointer is nullable, but at least one of obs, reward,
 *     terminated, truncated must be given.  What is written for step t of env i is what salp_robot_vec_step writes:
 *     inner_steps, the terminal row in final_obs (rows of finished envs only, the others are left as passed in), and with
 *     the same-step autoreset obs[t] holds the first row of the next episode.
 *   - the state rows are written back once, at the end of the launch; a later call continues where this one ended.
 *   - actions go through _rescale_action and the cycle-length guard of the env step unchanged: a cycle longer than the
 *     cut is cut there, and a non-finite length runs no Euler step.
 *   - results equal those of `horizon` salp_robot_vec_step calls up to what couples the lanes of a wavefront (the
 *     wave-uniform exact sin / cos and sqrt fallbacks, < 1e-12 relative per cycle): which lanes step together differs.
 *   - SALP_ERR_INVALID, nothing launched and the state untouched: a NULL handle, act or pol; horizon outside
 *     [1, SALP_ROBOT_MAX_ROLLOUT_CYCLES]; flag bits other than SALP_DEVICE_PTRS; obs, reward, terminated and truncated all
 *     NULL; a policy created on another handle; a dt the history calls refuse.  The cap bounds one launch on a shared GPU.
 *   - SALP_DEVICE_PTRS: the call only launches a kernel on `stream`: nothing is allocated or synchronised
 *     (graph-capturable).  Host pointers are staged (final_obs goes in as well as out) and the call returns after the
 *     stream is synchronised.
 * Policy (salp_robot_policy_*, salp_robot_vec_rollout_policy): the deterministic MLP of salp_vec.h "Policy" with obs_dim 6
 * and act_dim 3 — the same descriptor salp_policy_desc_t, the same public weight layout (per layer W[out][in] row-major,
 * then b[out]; then scale[3], shift[3]) and the same fixed fp32 arithmetic: every unit starts from its bias and adds its
 * inputs in index order with one fmaf each; relu; tanhf or the clamp to [-1, 1]; one multiply by scale, one add of shift.
 * The Gaussian head and sampled actions are declared in salp_robot_sampled.h, the evaluation form of the closed loop (one
 * summary record per robot and no per-step output) in salp_robot_evaluate.h.
 *   - the action of step 0 is the policy applied to the env's current observation: six float casts of the state, the row
 *     salp_robot_vec_reset with a zero mask returns.  The action of step t + 1 is the policy applied to the row written
 *     to obs[t] (after an autoreset: the first row of the new episode).  act_out (nullable) float [H][n][3] receives them.
 *   - n_policies > 1: env i runs policy i / (n / P); a wavefront never mixes policies, so P must divide n and n / P be a
 *     multiple of 64.  salp_robot_policy_words / _create return SALP_ERR_INVALID for a descriptor outside the ranges of
 *     salp_vec.h or such a P (words: the negative status), and for NULL arguments.
 *   - salp_robot_policy_update takes new weights of the same shape; with SALP_DEVICE_PTRS it is one kernel launch on
 *     `stream`: stream-ordered, nothing allocated (capturable).  With host pointers create and update return after the
 *     stream is synchronised.  A policy must be destroyed before its handle.
 */
#ifndef SALP_ROBOT_ROLLOUT_H
#define SALP_ROBOT_ROLLOUT_H
#include <stdint.h>
#include "salp_vec.h"     /* salp_policy_desc_t, the status codes, SALP_DEVICE_PTRS */
#include "salp_robot.h"   /* salp_robot_vec_t */
#ifdef __cplusplus
extern "C" {
#endif

enum { SALP_ROBOT_MAX_ROLLOUT_CYCLES = 1024 };   /* same reason as the trajectory cap: bounds one launch on a shared GPU */

/* horizon env steps (breathing cycles per robot) in ONE launch (see the top of this file): act float
 * [H][n][3]; obs float [H][n][6], reward float [H][n], terminated / truncated uint8 [H][n], final_obs float [H][n][6] (rows
 * of finished envs only), inner_steps int32 [H][n], each nullable but not all of the first four */
int salp_robot_vec_rollout(salp_robot_vec_t* h, const float* act, int32_t horizon, float* obs, float* reward,
                           uint8_t* terminated, uint8_t* truncated, float* final_obs, int32_t* inner_steps,
                           uint32_t flags, void* stream);

/* the in-kernel policy of salp_robot_vec_rollout_policy: salp_vec.h "Policy" with obs_dim 6 and act_dim 3 */
typedef struct salp_robot_policy salp_robot_policy_t;
/* float32 words of one policy in the public layout, or the negative status */
int salp_robot_policy_words(const salp_robot_vec_t* h, const salp_policy_desc_t* desc);
int salp_robot_policy_create(salp_robot_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags,
                             void* stream, salp_robot_policy_t** out);
int salp_robot_policy_update(salp_robot_policy_t* pol, const float* weights, uint32_t flags, void* stream);
void salp_robot_policy_destroy(salp_robot_policy_t* pol);

/* the same rollout with the actions computed in the kernel; act_out (nullable) float [H][n][3] */
int salp_robot_vec_rollout_policy(salp_robot_vec_t* h, const salp_robot_policy_t* pol, int32_t horizon, float* obs,
                                  float* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs,
                                  int32_t* inner_steps, float* act_out, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
