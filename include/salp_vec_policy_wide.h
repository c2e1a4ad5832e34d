/*
 * salp_vec_policy_wide.h — C ABI of the WIDE in-kernel policy: actors of up to 256 x 256 hidden units evaluated on the
 * matrix cores inside the one-food rollout kernels.  The handle, the policy object, the descriptor, the public weight
 * layout, the status codes and the flags are those of salp_vec.h; the functions are part of the same library.
 *
 *   salp_policy_words_wide            public words of one policy of a wide shape (negative: refused, salp_last_error says why)
 *   salp_policy_create_wide           a deterministic policy (salp_policy_create with the wide ranges)
 *   salp_policy_create_gaussian_wide  a Gaussian policy (salp_policy_create_gaussian with the wide ranges)
 *   salp_vec_last_launch_policy_wide  1 when the handle's most recent launch ran the wide kernels, else 0
 *
 * Why: salp_policy_create stops at two hidden layers of 64 units, the actor everybody trains (the reference's YAMLs, SB3's
 * MlpPolicy, this project's SACConfig) is 256 x 256.
 *
 * Shapes: n_hidden 1 or 2; every width a multiple of 32 in [32, 256] (unused entries 0); out_activation tanh or clip (a
 * Gaussian policy: tanh); n_policies under the rule of salp_vec.h (whole wavefronts per policy).  The handle must have
 * max_observed_food == 3 and num_food_items <= 1 (the one-food kernels); every other handle is refused at create with the
 * reason in salp_last_error.  `weights` is the public layout of salp_vec.h "Policy" / "Gaussian policy" (torch's nn.Linear
 * order), exactly as for the narrow create calls.
 *
 * The returned salp_policy_t is an ordinary one: salp_policy_update, salp_policy_set_noise_step, salp_policy_noise_step,
 * salp_policy_destroy and every run entry point — salp_vec_rollout_policy, _sampled, salp_vec_rollout_policy_packed,
 * _packed_sampled, salp_vec_evaluate_policy, _sampled, salp_vec_evaluate_navigation — accept it and run the wide
 * instantiation of their kernel.  Semantics, outputs, refusals and the noise stream are those of the narrow scheme.
 *
 * Arithmetic: the fixed order of salp_vec.h "Policy" — fp32, every unit starts from its bias and adds its inputs in
 * ascending index order with one fused multiply-add each — so a shape that both schemes accept gives the same bits under
 * either.  salp_vec_last_launch keeps reporting action source 2 (deterministic) or 3 (sampled).
 */
#ifndef SALP_VEC_POLICY_WIDE_H
#define SALP_VEC_POLICY_WIDE_H
#include <stdint.h>
#include "salp_vec.h"     /* salp_vec_t, salp_policy_t, salp_policy_desc_t, the status codes, SALP_DEVICE_PTRS */
#ifdef __cplusplus
extern "C" {
#endif

int salp_policy_words_wide(const salp_vec_t* h, const salp_policy_desc_t* desc, int gaussian);
int salp_policy_create_wide(salp_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags, void* stream,
                            salp_policy_t** out);
int salp_policy_create_gaussian_wide(salp_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags,
                                     void* stream, salp_policy_t** out);
int salp_vec_last_launch_policy_wide(const salp_vec_t* h);

#ifdef __cplusplus
}
#endif
#endif /* SALP_VEC_POLICY_WIDE_H */
