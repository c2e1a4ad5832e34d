/*
 * salp_robot_evaluate.h — C ABI of policy evaluation on the batched HEAD simulator: the closed-loop run of
 * salp_robot_vec_rollout_policy (salp_robot_rollout.h) or of its sampled form (salp_robot_sampled.h) with NO per-step
 * output — one summary record per robot, continuable across calls, with an optional stop at the end of each robot's first
 * episode.  The handle is the salp_robot_vec_t of salp_robot.h, the policy object the salp_robot_policy_t of
 * salp_robot_rollout.h; the status codes and SALP_DEVICE_PTRS are those of salp_vec.h, whose "Policy evaluation" this is
 * the robot's form of.  The functions are part of the same library.
 *
 * It replaces `out = rollout_policy(...); score = out.reward.sum(0)` where only totals per robot are wanted, and it is how a
 * policy is scored over whole episodes (the reference's test_robot.py: predict, step, stop at the episode's end, at most 500
 * cycles): with SALP_ROBOT_EVAL_FIRST_EPISODE a robot whose episode ended on cycle 12 does not simulate 488 more.
 *
 * Record.  rec is [n_envs][SALP_REVAL_WORDS] 32-bit words, 48 B per robot, contiguous; a device block must be 16-byte
 * aligned.  Integer words are stored as integers and the 64-bit fields are 8-byte aligned, so every field is a typed view
 * of the block.  Over the env steps a robot took in the call (and, with SALP_ROBOT_EVAL_ACCUMULATE, in the calls before):
 *   SALP_REVAL_RETURN (words 0-1, float64)        the sum of the step rewards AS THE float32 VALUES reward[t] of
 *                                                 salp_robot_vec_rollout_policy would hold, added in the robot's own step
 *                                                 order in fp64: a host loop `acc += (double)reward[t]` reproduces it bit
 *                                                 for bit
 *   SALP_REVAL_EULER_STEPS (words 4-5, int64)     the same sum over inner_steps[t]; simulated seconds = dt x this
 *   SALP_REVAL_FIRST_RETURN (words 2-3, float64), SALP_REVAL_FIRST_LENGTH (int32), SALP_REVAL_FIRST_EULER_STEPS (int32)
 *                                                 those two sums and the step count over the steps up to and including the
 *                                                 first step in which the robot finished (terminated or truncated); all
 *                                                 steps if it did not finish
 *   SALP_REVAL_FIRST_END (int32)                  0 the robot did not finish, 1 that first finishing step was terminated
 *                                                 (the target was reached, salp_robot_env.py:179), 2 truncated; terminated
 *                                                 wins
 *   SALP_REVAL_EPISODES (int32)                   steps with terminated or truncated set
 *   SALP_REVAL_REACHED (int32)                    steps with terminated set
 *   word 11                                       zero
 *
 * Flags: SALP_DEVICE_PTRS, SALP_ROBOT_EVAL_ACCUMULATE, SALP_ROBOT_EVAL_FIRST_EPISODE, in any combination.
 *   - SALP_ROBOT_EVAL_ACCUMULATE: the records are read first and continued: sums and counts go on, the FIRST_* fields stay
 *     frozen once FIRST_END != 0, an all-zero record is a fresh one.  Without the flag the records are overwritten.
 *   - SALP_ROBOT_EVAL_FIRST_EPISODE: a robot is no longer stepped once its first episode has ended.  The same-step autoreset
 *     of that last step has happened, so the robot sits at the start of its next episode with its draw counter one further.
 *     With SALP_ROBOT_EVAL_ACCUMULATE a robot whose record arrives with FIRST_END != 0 runs nothing: its record keeps every
 *     bit and its state rows are written back unchanged.  In this mode RETURN == FIRST_RETURN, EULER_STEPS ==
 *     FIRST_EULER_STEPS, EPISODES == (FIRST_END != 0) and REACHED == (FIRST_END == 1).
 * Records of rows >= n_envs are never touched.
 *
 * Everything else is salp_robot_vec_rollout_policy's (salp_robot_vec_evaluate_policy) or
 * salp_robot_vec_rollout_policy_sampled's (salp_robot_vec_evaluate_policy_sampled): which observation each action sees,
 * n_policies > 1, the service period of the handle, the horizon cap, the single state write-back at the end of the launch;
 * SALP_DEVICE_PTRS — the call only launches kernels on `stream`, allocates nothing and is capturable; host pointers are
 * staged, rec going in as well as out, and the call returns after the stream is synchronised; behind a sampled launch the
 * policy's noise step goes on by `horizon`, whichever robots stopped (the draw of a robot's step t is that of (env, n0 + t)).
 * The record equals, bit for bit, the fold above of what the rollout call writes for the same start and horizon.
 *
 * Continuation.  A run cut into several calls (SALP_ROBOT_EVAL_ACCUMULATE on every call but the first) equals one call in
 * every integer field; its float64 fields equal those of one call up to what couples the lanes of a wavefront
 * (salp_robot_rollout.h: lanes resynchronise at a call boundary, so which lanes step together differs).  The same sequence
 * of calls, eager or replayed from a captured graph, gives the same bits.
 *
 * SALP_ERR_INVALID, with nothing launched and the state, the noise step and rec untouched: a NULL h, pol or rec; horizon
 * outside [1, SALP_ROBOT_MAX_ROLLOUT_CYCLES]; flag bits other than the three above; a device rec that is not 16-byte
 * aligned; a policy created on another handle; the sampled call with a policy that is not Gaussian; a dt the history calls
 * refuse.
 */
#ifndef SALP_ROBOT_EVALUATE_H
#define SALP_ROBOT_EVALUATE_H
#include <stdint.h>
#include "salp_vec.h"             /* the status codes, SALP_DEVICE_PTRS */
#include "salp_robot.h"           /* salp_robot_vec_t */
#include "salp_robot_rollout.h"   /* salp_robot_policy_t, SALP_ROBOT_MAX_ROLLOUT_CYCLES */
#ifdef __cplusplus
extern "C" {
#endif

enum { SALP_ROBOT_EVAL_ACCUMULATE = 4u,      /* = SALP_EVAL_ACCUMULATE */
       SALP_ROBOT_EVAL_FIRST_EPISODE = 8u }; /* call flags next to SALP_DEVICE_PTRS (1u) */
enum { SALP_REVAL_RETURN = 0,             /* words 0-1: float64 */
       SALP_REVAL_FIRST_RETURN = 2,       /* words 2-3: float64 */
       SALP_REVAL_EULER_STEPS = 4,        /* words 4-5: int64 */
       SALP_REVAL_FIRST_LENGTH = 6, SALP_REVAL_FIRST_END = 7, SALP_REVAL_EPISODES = 8, SALP_REVAL_REACHED = 9,
       SALP_REVAL_FIRST_EULER_STEPS = 10, /* word 11: zero */
       SALP_REVAL_WORDS = 12 };           /* 48 B per robot */

/* rec: int32 [n_envs][SALP_REVAL_WORDS]; flags: SALP_DEVICE_PTRS, SALP_ROBOT_EVAL_ACCUMULATE, SALP_ROBOT_EVAL_FIRST_EPISODE */
int salp_robot_vec_evaluate_policy(salp_robot_vec_t* h, const salp_robot_policy_t* pol, int32_t horizon, void* rec,
                                   uint32_t flags, void* stream);
/* the same under the sampled actions of a Gaussian policy (salp_robot_sampled.h) */
int salp_robot_vec_evaluate_policy_sampled(salp_robot_vec_t* h, const salp_robot_policy_t* pol, int32_t horizon, void* rec,
                                           uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
