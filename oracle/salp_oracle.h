/*
 * salp_oracle.h — CPU restatement of the reference's SalpSnakeEnv (see salp_oracle.c).
 * TEST INFRASTRUCTURE ONLY: loaded by tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg; never by the product.  Uses the public POD config and the state-row
 * enums of include/salp_vec.h so snapshots are interchangeable with the HIP library's.
 */
#ifndef SALP_ORACLE_H
#define SALP_ORACLE_H
#include "../include/salp_vec.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct salp_oracle salp_oracle_t;

void salp_oracle_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
void salp_oracle_set_threads(int n);   /* OpenMP threads over envs; default 1 */
int salp_oracle_get_threads(void);

int salp_oracle_create(const salp_config_t* cfg, int64_t n_envs, uint64_t seed,
                       int64_t env_index_base, salp_oracle_t** out);
void salp_oracle_destroy(salp_oracle_t* h);
int salp_oracle_obs_dim(const salp_oracle_t* h);
int salp_oracle_act_dim(const salp_oracle_t* h);
int salp_oracle_reset(salp_oracle_t* h, const uint8_t* mask, float* obs);
int salp_oracle_observe(salp_oracle_t* h, float* obs);
/* reward64 (nullable) receives the un-rounded fp64 reward of the reference. */
int salp_oracle_step(salp_oracle_t* h, const float* act, float* obs, float* reward,
                     double* reward64, uint8_t* terminated, uint8_t* truncated, float* final_obs,
                     int32_t* info);
int salp_oracle_rollout(salp_oracle_t* h, const float* act, int32_t horizon, float* obs,
                        float* reward, double* reward64, uint8_t* terminated, uint8_t* truncated,
                        float* final_obs, int32_t* info, float* act_out);
/* test-only variant with fp64 actions (the reference accepts any float; the product ABI is f32) */
int salp_oracle_rollout_f64(salp_oracle_t* h, const double* act64, int32_t horizon, float* obs,
                            double* reward64, uint8_t* terminated, uint8_t* truncated);
int salp_oracle_get_state(salp_oracle_t* h, double* f64, int32_t* i32);
int salp_oracle_set_state(salp_oracle_t* h, const double* f64, const int32_t* i32);
int64_t salp_oracle_global_step(const salp_oracle_t* h);
int salp_oracle_set_base_num_food(salp_oracle_t* h, int k);   /* snake:36 base_num_food_items, 0..num_food_items */
/* Food placement counters, per env since creation or the last clear; they change no output.  out: int64 [SALP_ORACLE_PC_COUNT][n]. */
enum {
  SALP_ORACLE_PC_RESET_PLACED = 0,         /* foods placed at reset (create, reset with or without a mask, autoreset) */
  SALP_ORACLE_PC_RESET_FORCED = 1,         /* ... of them by the unconditional draw behind `reset_limit` rejections */
  SALP_ORACLE_PC_RESPAWN_PLACED = 2,       /* foods placed at respawn */
  SALP_ORACLE_PC_RESPAWN_FORCED = 3,       /* ... of them by the unconditional draw behind `respawn_limit` rejections */
  SALP_ORACLE_PC_MAX_VALID_REJECTIONS = 4, /* the most rejections that preceded a VALID acceptance */
  SALP_ORACLE_PC_COUNT = 5
};
int salp_oracle_get_placement_counters(const salp_oracle_t* h, int64_t* out);
int salp_oracle_clear_placement_counters(salp_oracle_t* h);
/* The rejection limits (snake:99 and :239; defaults 100 and 50) of LATER resets and respawns: test guard only. */
int salp_oracle_set_placement_limits(salp_oracle_t* h, int reset_limit, int respawn_limit);
/* The in-kernel policy (include/salp_vec.h "Policy") in the header's own arithmetic, from the public weight layout of
 * ONE policy: obs [M][obs_dim] -> u [M][act_dim] (nullable; before the output activation) and a [M][act_dim].
 * subnormals (nullable): the number of non-zero subnormal values formed on the way.  See salp_oracle.c. */
int salp_oracle_policy_forward(const salp_policy_desc_t* desc, int32_t obs_dim, int32_t act_dim, const float* weights,
                               const float* obs, int64_t M, float* u, float* a, int64_t* subnormals);
/* The two heads of a Gaussian policy from the public Gaussian layout of ONE policy (hidden layers, W_mu, b_mu, W_ls, b_ls,
 * scale, shift): m [M][act_dim] the mean head, r [M][act_dim] the log-std head's raw sum before its clamp. */
int salp_oracle_policy_forward_gaussian(const salp_policy_desc_t* desc, int32_t obs_dim, int32_t act_dim, const float* weights,
                                        const float* obs, int64_t M, float* m, float* r, int64_t* subnormals);
#ifdef __cplusplus
}
#endif
#endif
