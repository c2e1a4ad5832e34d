/*
 * salp_vec.h — C ABI of the batched SALP swimmer simulator for AMD MI355X (gfx950).
 *
 * One handle (`salp_vec_t`) owns the struct-of-arrays state of `n_envs` independent
 * SalpSnakeEnv instances on ONE GPU and advances all of them with one fused HIP kernel
 * per call.  The entry points are what a binding of the reference's Gymnasium `Env`
 * surface needs — the reference has no FFI of its own, so each one cites the reference
 * method it replaces (paths relative to the reference repo; "legacy" =
 * scripts/utilities/salp_robot.py, "snake" = src/salp/environments/salp_snake_env.py):
 *
 *   salp_config_default     snake:29-33 (the 13 constructor kwargs) + legacy:32-53 (constants)
 *   salp_vec_create         SalpSnakeEnv.__init__            snake:29-90
 *   salp_vec_reset          SalpSnakeEnv.reset               snake:133-155, legacy:95-117
 *   salp_vec_step           SalpSnakeEnv.step                snake:157-202, legacy:119-156
 *   salp_vec_rollout        the caller's `for t in range(T): env.step(a[t])` loop
 *                           (train.py:110-122, eval/collect_navigation_data.py:97-114)
 *   salp_vec_step_packed / salp_vec_rollout_packed
 *                           the same two with the returned tuple (obs, reward, terminated, truncated, info) packed
 *                           into one record per env and step — no reference counterpart
 *   salp_vec_get/set_state  attribute pokes `env.robot_pos = …`, `env.food_positions = …`
 *                           (eval/collect_navigation_data.py:76-89) and legacy:390-403 (_get_info)
 *   salp_vec_observe        SalpSnakeEnv._get_extended_observation   snake:366-428
 *
 * Conventions
 *   - every function returns 0 (SALP_OK) or a negative salp_status; the message for the
 *     calling thread's last failure is `salp_last_error()`.  Nothing throws or aborts.
 *   - every data buffer is caller-owned.  `flags & SALP_DEVICE_PTRS` says the data
 *     pointers are device pointers on the handle's GPU; the call is then asynchronous on
 *     `stream` (a hipStream_t passed as void*, NULL = the null stream).  Without the flag the
 *     pointers are host pointers and the call is synchronous (H2D, kernel, D2H inside).
 *   - a handle is not thread-safe; distinct handles (one per GPU) are independent.
 *   - every call runs on the handle's device and leaves the caller's current HIP device as it found it.
 *   - there is no CPU fallback: creating a handle without a usable HIP device fails with
 *     SALP_ERR_NO_DEVICE.
 *
 * Randomness (the reference uses two global un-seeded Mersenne Twisters — snake:12 `random`,
 * legacy:311 `np.random` — so its draws are not reproducible; this library defines them):
 *   block(env, n) = Philox4x32-10(counter = (env_lo, env_hi, n, 0), key = (seed_lo, seed_hi))
 *   where env is the GLOBAL env index (env_index_base + local index) and n is that env's
 *   running draw counter (state row SALP_I_RNG_COUNTER).  Each draw EVENT consumes one block,
 *   in program order of the reference:
 *     thrust jitter  (legacy:311)                u = u53(w0,w1)
 *     one food-placement attempt (snake:101-104, 127-130, 239-242, 269-272)
 *                                                x = lo+(hi-lo)*u53(w0,w1), y likewise from (w2,w3)
 *     random food count (snake:146)              1 + ((w0 * n) >> 32)
 *   u53(a,b) = ((a>>5)*2^26 + (b>>6)) / 2^53.
 *   Device-generated actions (salp_vec_rollout with act == NULL): with t = the handle's global step
 *   count and j the action component,
 *     w = word (t & 3) of Philox4x32-10(counter = (env_lo, env_hi, t >> 2, 1 + j), key)
 *     a_j = (w >> 8) * 2^-23 - 1   in [-1, 1)      (nozzle direction)
 *     a_0 = (w >> 8) * 2^-24       in [0, 1)       (inhale control, 2-action mode only)
 *   (one block serves four consecutive steps of a component).
 *   Policy noise (salp_vec_rollout_policy_sampled, salp_vec_evaluate_policy_sampled; "Sampled actions" below):
 *     block(env, n) = Philox4x32-10(counter = (env_lo, env_hi, n, 3), key)
 *   env is the global env index, n the low 32 bits of the policy's noise step for that env-step (the fourth counter word
 *   separates the streams: 0 env draws, 1 and 2 device action streams, 3 policy noise).  The env's own draw counter
 *   (SALP_I_RNG_COUNTER) is not consumed: the simulator's trajectory stays a function of the actions alone.
 *   Action component j takes one standard normal draw from words (w[2j], w[2j+1]) of the one block, fp32 (Box-Muller):
 *     u1 = ((w[2j] >> 8) + 1) * 2^-24   in (0, 1]       u2 = (w[2j+1] >> 8) * 2^-24   in [0, 1)
 *     z  = sqrtf(-2 * logf(u1)) * cospif(2 * u2)         (cospif, the device library's cos(pi x), is the one used)
 *   The noise step is a 64-bit device word owned by the policy object: the kernels read it at entry (the action of step t
 *   of a call uses n0 + t), and a one-thread kernel enqueued behind the call's launches adds `horizon` — so a replayed
 *   hipGraph draws fresh noise.  salp_policy_create_gaussian starts it at 0; salp_vec_reseed re-keys the stream (the key
 *   is the handle's) and leaves the step alone.
 */
#ifndef SALP_VEC_H
#define SALP_VEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SALP_ABI_VERSION 1
#define SALP_MAX_FOOD 16        /* num_food_items upper bound (sac_gail.yaml uses 12) */
#define SALP_MAX_OBSERVED_FOOD 8

typedef enum salp_status {
  SALP_OK = 0,
  SALP_ERR_INVALID = -1,    /* bad argument / config */
  SALP_ERR_NO_DEVICE = -2,  /* no HIP device, or device_id out of range */
  SALP_ERR_HIP = -3,        /* a HIP runtime call failed */
  SALP_ERR_OOM = -4
} salp_status;

enum { SALP_DEVICE_PTRS = 1u };
enum { SALP_REC_FINAL_OBS = 2u };   /* salp_vec_step_packed / salp_vec_rollout_packed: records carry the terminal observation */

/* POD of the reference's parameters.  Units are the reference's (pixels, steps, radians). */
typedef struct salp_config {
  uint32_t struct_size;            /* = sizeof(salp_config_t); checked by salp_vec_create */
  /* snake:29-33 kwargs */
  int32_t width;                   /* 800 */
  int32_t height;                  /* 600 */
  int32_t num_food_items;          /* 5   (base_num_food_items, snake:36) */
  int32_t max_observed_food;       /* 3   (K; obs_dim = 10 + 4K + 2, snake:79-80) */
  int32_t max_steps_without_food;  /* 1500 */
  int32_t forced_breathing;        /* 1   (act_dim 1; 0 -> act_dim 2, snake:69-74) */
  int32_t random_food_count;       /* 0 */
  int32_t respawn_food;            /* 1 */
  double food_reward;              /* 10.0 */
  double collision_penalty;        /* -50.0 */
  double time_penalty;             /* -0.1 */
  double efficiency_bonus;         /* 1.0 */
  double proximity_reward_weight;  /* 0.0 */
  /* legacy:32-53 constants and snake:53-54 */
  double tank_margin;              /* 50 */
  double base_radius;              /* 30 */
  double max_thrust_force;         /* 100 */
  double drag_coefficient;         /* 0.98 */
  double angular_drag;             /* 0.95 (literal at legacy:320) */
  double max_nozzle_angle;         /* pi/3 */
  double nozzle_response_rate;     /* 0.05 */
  double food_radius;              /* 15 */
  double min_food_distance;        /* 80 */
  int32_t inhale_duration;         /* 120 */
  int32_t exhale_duration;         /* 150 */
  int32_t rest_duration;           /* 60 (enters only through the 330-step modulus, legacy:161) */
  int32_t no_autoreset;            /* 0: an env that terminates or truncates starts its next episode in the same step
                                    * (VectorEnv convention).  1: it is NOT reset, exactly like the reference's single env
                                    * when its caller ignores `done` and keeps stepping (eval/collect_navigation_data.py:
                                    * 97-114 rides through wall contacts this way); flags are still reported each step. */
} salp_config_t;

/* Rows of the state snapshot exchanged by salp_vec_get_state / salp_vec_set_state.
 * f64 block: [SALP_F_COUNT(F)][n_envs] doubles, row-major (one row per quantity).
 * i32 block: [SALP_I_COUNT][n_envs] int32.
 * A collected / absent food slot (`None` in snake:215) is NaN in both coordinates. */
enum {
  SALP_F_X = 0, SALP_F_Y, SALP_F_VX, SALP_F_VY, SALP_F_THETA, SALP_F_OMEGA,
  SALP_F_NOZZLE, SALP_F_WATER,
  SALP_F_ELLIPSE_A, SALP_F_ELLIPSE_B,   /* derived on get; ignored on set */
  SALP_F_FOOD0                          /* then food_x[0..F-1], food_y[0..F-1] */
};
#define SALP_F_COUNT(F) (SALP_F_FOOD0 + 2 * (F))
enum {
  SALP_I_PHASE = 0,        /* 0 rest, 1 inhaling, 2 exhaling (legacy:374) */
  SALP_I_TIMER,            /* breathing_timer */
  SALP_I_EXHALE_DUR,       /* current_exhale_duration (legacy:223) */
  SALP_I_SHAPE_HOLD,       /* 0 = ellipse follows (phase,timer,dur,water); 7 = post-reset circle
                              (a=b=base_radius, legacy:112-113); 1..6 = inhale timer at an early
                              release that returned to rest (legacy:225-228 keeps the old a,b) */
  SALP_I_STEPS_SINCE_FOOD,
  SALP_I_FOOD_COLLECTED,
  SALP_I_RNG_COUNTER,      /* next Philox block index of this env */
  SALP_I_EPISODE_LENGTH,
  SALP_I_COUNT
};

/* Ranges accepted by salp_vec_set_state.  The reference takes any attribute poke; this library packs the breathing integers
 * into one word and wraps the heading in a bounded loop, so a snapshot must lie where the kernels and the reference agree:
 *   SALP_F_WATER            in [0, 1] (not NaN).  The reference only ever produces t / inhale_duration and its decay; the
 *                           literal-constant kernels take ellipse_a for max(ellipse_a, ellipse_b), which holds on [0, 1] only,
 *                           and a released breath lasts int(exhale_duration * max(water, 0.3)) <= 255 steps only there.
 *   SALP_F_THETA, _OMEGA    finite, |value| <= SALP_SET_STATE_MAX_ANGLE (100 rad, rad/step).  An unwrapped heading is observed
 *                           as it is (theta / pi, as snake:392 would) and wrapped to [-pi, pi] by the next step exactly as
 *                           legacy:329-332 does; fp32 keeps theta / pi and the food bearings to 1e-5 up to this magnitude.
 *   SALP_I_PHASE 0..2, SALP_I_TIMER 0..255, SALP_I_EXHALE_DUR 0..255, SALP_I_SHAPE_HOLD 0..7   (the packed word's fields).
 * With host pointers a snapshot outside these ranges is refused as a whole (SALP_ERR_INVALID, the message names the first
 * offending env; no env is written).  With SALP_DEVICE_PTRS the call is asynchronous and cannot look at the data: the ranges
 * are then the caller's obligation.  Positions, velocities, the nozzle angle and the counters are taken as given. */
#define SALP_SET_STATE_MAX_ANGLE 100.0

/* Per-step info columns (int32 [n_envs][SALP_INFO_COLS]); values are those of the step's own
 * (pre-autoreset) episode, as in the info dict of snake:195-200. */
enum { SALP_INFO_FOOD_COLLECTED = 0, SALP_INFO_STEPS_SINCE_FOOD, SALP_INFO_COLLISION, SALP_INFO_COLS };

/* Packed transition record (salp_vec_step_packed / salp_vec_rollout_packed): everything a step returns as ONE row of 32-bit
 * words per env and step, so that a consumer hands one block on (a collective, a replay buffer) instead of six streams.
 * With OD = obs_dim:
 *   words 0 .. OD-1     the observation, float32: what `obs` of salp_vec_step receives (post-autoreset)
 *   word  OD + SALP_REC_REWARD             reward, float32
 *   word  OD + SALP_REC_FLAGS              byte 0 terminated (0/1), byte 1 truncated (0/1), byte 2 collision (0/1), byte 3 zero
 *   word  OD + SALP_REC_FOOD_COLLECTED     int32, SALP_INFO_FOOD_COLLECTED of the step (pre-autoreset episode)
 *   word  OD + SALP_REC_STEPS_SINCE_FOOD   int32, likewise
 * and, with the call flag SALP_REC_FINAL_OBS, OD more words: the terminal observation of an env that finished in that
 * step; in the rows of unfinished envs those words are not written (the final_obs rule of salp_vec_step).  Integer words are
 * stored as integers, so every field is a typed view of the block (bytes 0 and 1 of the flags word are bool arrays).
 * A block is [horizon][n_envs][salp_vec_record_width] words, contiguous; a device block must be 16-byte aligned. */
enum { SALP_REC_REWARD = 0, SALP_REC_FLAGS, SALP_REC_FOOD_COLLECTED, SALP_REC_STEPS_SINCE_FOOD, SALP_REC_EXTRA_COLS };

/* Running totals since create / salp_vec_clear_stats, reduced on the device
 * (wave-shuffle + one atomic per wave; fixed-point so the sum is order-independent). */
typedef struct salp_stats {
  int64_t env_steps;          /* env-steps simulated */
  int64_t episodes;           /* episodes finished (terminated | truncated) */
  int64_t terminated;
  int64_t truncated;
  int64_t collisions;
  int64_t food_collected;
  int64_t episode_length_sum; /* over finished episodes */
  double reward_sum;          /* over all env-steps (accumulated in 2^-20 fixed point) */
  double episode_return_sum;  /* over finished episodes (2^-20 fixed point) */
} salp_stats_t;

typedef struct salp_vec salp_vec_t;

const char* salp_last_error(void);
int salp_abi_version(void);
int salp_device_count(void);

/* Fills *cfg with the reference defaults (snake:29-33, legacy:32-53). */
int salp_config_default(salp_config_t* cfg);

/* device_id: HIP ordinal.  env_index_base: global index of local env 0 (multi-GPU sharding keeps
 * env i's trajectory independent of the number of shards).  The handle starts in the post-reset
 * state of every env (draw counters at 0 before that reset). */
int salp_vec_create(const salp_config_t* cfg, int64_t n_envs, int device_id, uint64_t seed,
                    int64_t env_index_base, salp_vec_t** out);
void salp_vec_destroy(salp_vec_t* h);

int64_t salp_vec_num_envs(const salp_vec_t* h);
int salp_vec_obs_dim(const salp_vec_t* h);   /* 10 + 4K + 2 */
int salp_vec_act_dim(const salp_vec_t* h);   /* 1 (forced breathing) or 2 */
int salp_vec_num_food(const salp_vec_t* h);  /* F */
int salp_vec_device(const salp_vec_t* h);

/* reset(): mask == NULL resets every env, else the envs with mask[i] != 0.
 * obs (may be NULL): float [n_envs][obs_dim]; rows of envs that were not reset are written with
 * their current observation. */
int salp_vec_reset(salp_vec_t* h, const uint8_t* mask, float* obs, uint32_t flags, void* stream);

/* step(): act float [n_envs][act_dim] (not clipped, as in the reference).
 * obs float [n_envs][obs_dim]; reward float [n_envs]; terminated, truncated uint8 [n_envs].
 * Autoreset is same-step: a finished env is reset inside the call and `obs` holds the first
 * observation of its next episode; its terminal observation goes to final_obs (float
 * [n_envs][obs_dim], rows of unfinished envs untouched) when that pointer is non-NULL.
 * info (may be NULL): int32 [n_envs][SALP_INFO_COLS]. */
int salp_vec_step(salp_vec_t* h, const float* act, float* obs, float* reward,
                  uint8_t* terminated, uint8_t* truncated, float* final_obs, int32_t* info,
                  uint32_t flags, void* stream);

/* rollout(): horizon steps in ONE kernel launch, state held in registers across steps.
 * act float [horizon][n_envs][act_dim], or NULL for device-generated U[-1,1) actions
 * (then act_out, if non-NULL, receives them).  obs float [horizon][n_envs][obs_dim];
 * reward float [horizon][n_envs]; terminated / truncated uint8 [horizon][n_envs].
 * Any of obs / reward / terminated / truncated may be NULL (not written).
 * final_obs as in step(), shaped [horizon][n_envs][obs_dim] (may be NULL). */
int salp_vec_rollout(salp_vec_t* h, const float* act, int32_t horizon, float* obs, float* reward,
                     uint8_t* terminated, uint8_t* truncated, float* final_obs, float* act_out,
                     uint32_t flags, void* stream);

/* Words per record: obs_dim + SALP_REC_EXTRA_COLS, or 2 obs_dim + SALP_REC_EXTRA_COLS with SALP_REC_FINAL_OBS in flags. */
int salp_vec_record_width(const salp_vec_t* h, uint32_t flags);

/* step() / rollout() with the packed record as the only output ("Packed transition record" above): rec is
 * [n_envs][width] / [horizon][n_envs][width] words.  flags: SALP_DEVICE_PTRS and / or SALP_REC_FINAL_OBS.  act, act_out, the
 * global step, the statistics and the same-step autoreset are those of salp_vec_step / salp_vec_rollout (act == NULL:
 * device-generated actions, rollout only).  With device pointers the call only launches kernels on `stream` (capturable
 * into a hipGraph, like salp_vec_step).  SALP_ERR_INVALID, with nothing launched and the handle unchanged, for a NULL
 * rec, horizon < 1, a flag bit other than those two, or a device rec that is not 16-byte aligned. */
int salp_vec_step_packed(salp_vec_t* h, const float* act, float* rec, uint32_t flags, void* stream);
int salp_vec_rollout_packed(salp_vec_t* h, const float* act, int32_t horizon, float* rec, float* act_out,
                            uint32_t flags, void* stream);

/* Policy: a small MLP evaluated INSIDE the rollout kernel, so that a closed-loop rollout (every action a function of the
 * previous observation) is one launch — no reference counterpart; it replaces the caller's
 * `for t: a = actor(obs); obs = env.step(a)` loop (train.py:110-122 with the actor of the SAC trainer).
 * The function, for an observation row x (obs_dim floats):
 *   h = relu(W x + b) for each hidden layer;  u = W_last h + b_last;  a = act(u) * scale + shift,
 *   act = tanhf (SALP_POLICY_OUT_TANH) or a clamp to [-1, 1] (SALP_POLICY_OUT_CLIP).
 * Weights of ONE policy, float32, `salp_policy_words` words — the layout of torch's nn.Linear: for each layer in order
 * W[out][in] row-major, then b[out] (the last layer has out = act_dim); then scale[act_dim], shift[act_dim].
 * A block of P policies is [P][words].  The library re-lays the block into a buffer of its own at create / update.
 * Arithmetic: fp32 throughout, in one fixed order in every kernel: each unit starts from its bias and adds its inputs in
 * index order with one fused multiply-add each (fmaf(w, x, acc)); relu = fmaxf(acc, 0); then tanhf or the clamp; then one
 * multiply by scale and one add of shift (two roundings).  An action is a deterministic function of (weights, observation).
 * Policy assignment: P == 1: every env runs the one policy, for any n_envs.  P > 1: env i runs policy i / (n_envs / P);
 * n_envs % P == 0 and (n_envs / P) % 64 == 0 are required (a wavefront never mixes policies). */
enum { SALP_POLICY_OUT_TANH = 0, SALP_POLICY_OUT_CLIP = 1 };
typedef struct salp_policy_desc {
  uint32_t struct_size;     /* = sizeof(salp_policy_desc_t) */
  int32_t  n_hidden;        /* 0, 1 or 2 hidden layers (0 = linear policy) */
  int32_t  hidden[2];       /* each a multiple of 16 in [16, 64]; unused entries 0 */
  int32_t  out_activation;  /* SALP_POLICY_OUT_TANH or SALP_POLICY_OUT_CLIP */
  int32_t  n_policies;      /* P >= 1 */
} salp_policy_desc_t;
typedef struct salp_policy salp_policy_t;

/* float32 words of ONE policy of this shape on this handle, or a negative salp_status (descriptor out of range). */
int salp_policy_words(const salp_vec_t* h, const salp_policy_desc_t* desc);
/* A policy bound to the handle's device, obs_dim, act_dim and n_envs (handles with max_observed_food == 3 only).
 * weights: [P][words], host pointers, or device pointers with SALP_DEVICE_PTRS (then asynchronous on `stream`).
 * SALP_ERR_INVALID for a descriptor outside the ranges above or a P that n_envs does not allow.  Destroy the policy before
 * its handle. */
int salp_policy_create(salp_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags, void* stream,
                       salp_policy_t** out);
/* New weights of the same shape.  With SALP_DEVICE_PTRS the call is stream-ordered and allocates nothing: it may sit between
 * two replays of a captured graph that holds salp_vec_rollout_policy calls, which then run the new weights. */
int salp_policy_update(salp_policy_t* pol, const float* weights, uint32_t flags, void* stream);
void salp_policy_destroy(salp_policy_t* pol);

/* Gaussian policy: the stochastic actor of the learners (sac.Actor: mean and log-std heads on one body, tanh squashing).
 * Weights of ONE policy, float32, `salp_policy_words_gaussian` words: the hidden layers as above; then the mean head
 * W_mu[A][in], b_mu[A]; then the log-std head W_ls[A][in], b_ls[A]; then scale[A], shift[A].  out_activation must be
 * SALP_POLICY_OUT_TANH; the other ranges (0-2 hidden layers of 16..64 units, K = 3 handles, P and n_envs) are those of
 * salp_policy_create.  The result is an ordinary salp_policy_t: salp_policy_update takes the Gaussian layout for it, and
 * salp_vec_rollout_policy / salp_vec_evaluate_policy run its MEAN — every output equals, bit for bit, that of the plain
 * policy built from the same body and mean head. */
int salp_policy_words_gaussian(const salp_vec_t* h, const salp_policy_desc_t* desc);
int salp_policy_create_gaussian(salp_vec_t* h, const salp_policy_desc_t* desc, const float* weights, uint32_t flags, void* stream,
                                salp_policy_t** out);
/* The noise step of a Gaussian policy ("Randomness").  set: stream-ordered (a one-thread kernel on `stream`).  get: waits for
 * the stream of the policy's most recent create / update / set / sampled call, then reads the word with a blocking copy — so
 * it must not be called while a stream is capturing.  Ordering is stream ordering and nothing else: salp_policy_set_noise_step
 * and the sampled calls that are to see its value must be issued on the same stream (or on streams the caller has ordered).
 * The sampled entry points take the policy as const and still advance this word on the device: a salp_policy_t is not
 * thread-safe, like the handle it is bound to.  SALP_ERR_INVALID for a policy that is not Gaussian. */
int salp_policy_set_noise_step(salp_policy_t* pol, uint64_t n, void* stream);
int salp_policy_noise_step(salp_policy_t* pol, uint64_t* n);

/* Sampled actions: salp_vec_rollout_policy / salp_vec_evaluate_policy with the stochastic form of a Gaussian policy.  Per
 * action component j, fp32, in one fixed order in every kernel (z_j: the draw of "Randomness" for this env and noise step):
 *   mu = mean head (the deterministic arithmetic above);  ls = the log-std head in the same fmaf order, then
 *   ls = fminf(fmaxf(ls, -20), 2);  sd = expf(ls);  u = fmaf(sd, z, mu);  a = tanhf(u) * scale + shift   (two roundings)
 *   m = -2 * u;  sp = fmaxf(m, 0) + log1pf(expf(-fabsf(m)));  c = (log 2 - u) - sp
 *   g = -0.5 * (z * z);  g = g - ls;  g = g - 0.5 log(2 pi);  g = g - 2 * c;      logp = 0 + g_0 (+ g_1), in index order
 * — sac.Actor.forward's value with (u - mu) / std taken as z.  Every operation above is one fp32 rounding (no contraction).
 * Which observation each action sees (the bit-exact prologue row included), P > 1 assignment, autoreset, state write-back,
 * global step, statistics, the split launch for ragged n, device / host pointers and capturability are those of the
 * deterministic twins.  logp_out (may be NULL): float [horizon][n_envs]; act_out may be NULL.  After the launches the policy's
 * noise step has advanced by `horizon` (on the device, stream-ordered; if that last one-thread launch itself fails the call
 * returns the HIP error with the envs stepped and the noise step not advanced: set it before sampling on).
 * SALP_ERR_INVALID, with nothing launched and the handle and the noise step unchanged, for a policy that is not Gaussian
 * and for everything the deterministic twin refuses. */
int salp_vec_rollout_policy_sampled(salp_vec_t* h, const salp_policy_t* pol, int32_t horizon, float* obs, float* reward,
                                    uint8_t* terminated, uint8_t* truncated, float* act_out, float* logp_out,
                                    uint32_t flags, void* stream);
int salp_vec_evaluate_policy_sampled(salp_vec_t* h, const salp_policy_t* pol, int32_t horizon, void* rec,
                                     uint32_t flags, void* stream);

/* rollout() with the actions computed in the kernel: the action of step 0 is the policy applied to the env's current
 * observation; the action of step t + 1 is the policy applied to the row written to obs[t] (after a same-step autoreset
 * the first observation of the new episode; with no_autoreset the row as returned).
 * When the state was left by a step, the observation of step 0 is formed with the bits of that step's row, so a rollout
 * cut into several calls takes the same actions, bit for bit, as one call.  For a state that no step left (reset,
 * set_state) it is the row salp_vec_observe returns up to the last bits of ONE column: the relative bearing of the nearest
 * food (column 13) goes through the step's arctangent polynomial or through salp_vec_observe's, which differ by a few units
 * in the last place (as a step's own row and salp_vec_observe after it do).
 * obs, reward, terminated, truncated as in salp_vec_rollout, all four required; act_out (may be NULL) receives the actions
 * taken, float [horizon][n_envs][act_dim].  Global step, statistics, state write-back and autoreset are those of
 * salp_vec_rollout.  With device pointers the call only launches kernels on `stream` (capturable).
 * SALP_ERR_INVALID, with nothing launched and the handle unchanged, for a policy of another handle or other dimensions,
 * horizon < 1, a NULL main output, or a P that n_envs does not allow. */
int salp_vec_rollout_policy(salp_vec_t* h, const salp_policy_t* pol, int32_t horizon, float* obs, float* reward,
                            uint8_t* terminated, uint8_t* truncated, float* act_out, uint32_t flags, void* stream);

/* Policy evaluation: the closed-loop run of salp_vec_rollout_policy with NO per-step output — one summary record per env,
 * [n_envs][SALP_EVAL_WORDS] 32-bit words (32 B per env; a device block must be 16-byte aligned), covering the `horizon` steps
 * of the call.  It replaces `out = rollout_policy(...); score = out.reward.sum(0)` where only totals per env are wanted (the
 * reference evaluates this way: test_model.py, eval/collect_navigation_data.py run_single_trial keep totals per episode).
 *   SALP_EVAL_RETURN (words 0-1, float64)        the sum of the step rewards AS THE float32 VALUES reward[t] of
 *                                                salp_vec_rollout_policy would hold, added in step order in fp64: a host loop
 *                                                `acc += (double)reward[t]` reproduces it bit for bit
 *   SALP_EVAL_FIRST_RETURN (words 2-3, float64), SALP_EVAL_FIRST_LENGTH (int32)
 *                                                the same sum and the step count over the steps up to and including the first
 *                                                step in which the env finished (terminated or truncated); all steps if it did not
 *   SALP_EVAL_FIRST_END (int32)                  0 the env did not finish, 1 that first finishing step was terminated, 2 truncated
 *                                                (terminated wins, as in salp_stats_t)
 *   SALP_EVAL_EPISODES (int32)                   steps in which the env finished (with no_autoreset: every flagged step)
 *   SALP_EVAL_FOOD (int32)                       steps with a capture
 * Integer words are stored as integers and the float64 fields are 8-byte aligned: every field is a typed view of the block.
 * flags: SALP_DEVICE_PTRS and / or SALP_EVAL_ACCUMULATE.  With SALP_EVAL_ACCUMULATE the records are read first and continued:
 * sums and counts go on, the FIRST_* fields stay frozen once FIRST_END != 0, an all-zero record is a fresh one — a run cut
 * into several calls, or replayed from a captured graph, yields the bits of one call.  Without it the records are overwritten.
 * Which observation each action sees (the prologue's bit-exact row included), the policy assignment for P > 1, the state
 * write-back, autoreset, global step and statistics are those of salp_vec_rollout_policy.  Host pointers: synchronous; device
 * pointers: the call only launches kernels on `stream` (capturable).
 * SALP_ERR_INVALID, with nothing launched and the handle unchanged, for a NULL rec, horizon < 1, a flag bit other than those
 * two, a device rec that is not 16-byte aligned, a policy of another handle or other dimensions, or a P that n_envs does not
 * allow. */
enum { SALP_EVAL_ACCUMULATE = 4u };
enum { SALP_EVAL_RETURN = 0,        /* words 0-1: float64 */
       SALP_EVAL_FIRST_RETURN = 2,  /* words 2-3: float64 */
       SALP_EVAL_FIRST_LENGTH = 4, SALP_EVAL_FIRST_END, SALP_EVAL_EPISODES, SALP_EVAL_FOOD, SALP_EVAL_WORDS /* 8 */ };
int salp_vec_evaluate_policy(salp_vec_t* h, const salp_policy_t* pol, int32_t horizon, void* rec, uint32_t flags, void* stream);

/* Navigation evaluation: fixed start -> goal trials (the reference's eval/collect_navigation_data.py :97-114) in ONE launch —
 * the closed loop of salp_vec_rollout_policy with a per-env stop at the goal, NO per-step output but the optional track, and
 * one path record per env, [n_envs][SALP_NAV_WORDS] 32-bit words (80 B per env; a device block must be 16-byte aligned).
 *   line          double [n_envs][4]: start x, start y, goal x, goal y of each env's trial (the caller has put the envs at
 *                 their starts with salp_vec_set_state; the start here only defines the line of the lateral deviation)
 *   goal_radius   one double for the whole call
 * An env is RUNNING while the reached bit of its record is clear.  An env that is not running is not stepped: its state rows,
 * draw counter, statistics and record keep every bit.  After each step a running env takes, in fp64 with IEEE sqrt and
 * division and no contraction — a host loop reproduces every bit — with (x, y) the state position after the step (wall clamp
 * included) and (px, py) the one before it:
 *   path_sum += sqrt((x-px)*(x-px) + (y-py)*(y-py))
 *   lateral_sum += fabs((x-sx)*dny - (y-sy)*dnx),  (dnx, dny) = (gx-sx, gy-sy) / (sqrt((gx-sx)^2 + (gy-sy)^2) + 1e-12)
 *   xmin = fmin(xmin, x) ... ymax = fmax(ymax, y);  steps += 1
 *   status |= 2 if the step collided, |= 4 if it captured the food
 *   status |= 1 if sqrt((x-gx)*(x-gx) + (y-gy)*(y-gy)) < goal_radius: the env stops running
 * The goal is tested after a step only: an env that starts inside the radius still takes one step.  `terminated` /
 * `truncated` do not end a trial (the reference's loop ignores them), hence the handle must have no_autoreset.
 *   SALP_NAV_STEPS (word 0, int32)          steps taken
 *   SALP_NAV_STATUS (word 1, int32)         bit 0 reached, bit 1 collided on a step taken, bit 2 captured the food
 *   SALP_NAV_PATH (words 2-3, float64)      path_sum
 *   SALP_NAV_LATERAL (words 4-5, float64)   lateral_sum over steps 1..steps (the term of the start itself is exactly 0)
 *   SALP_NAV_XMIN, _XMAX, _YMIN, _YMAX (words 6-13, float64)   the bounding box of the positions, the entry position included
 *   SALP_NAV_X, SALP_NAV_Y (words 14-17, float64)              the last position (= the state's)
 *   words 18-19                             zero
 * A fresh record: steps, status and the sums 0, the box and the last position the entry position.  flags: SALP_DEVICE_PTRS
 * and / or SALP_EVAL_ACCUMULATE.  With SALP_EVAL_ACCUMULATE the records are read first and continued; a record with steps == 0
 * and status == 0 counts as fresh — a run cut into several calls, or replayed from a captured graph, yields the bits of one
 * call.  Without it the records are overwritten.
 * track_or_null: double [horizon][n_envs][2], the position after each step of THIS call; a stopped env repeats its last one.
 * Which observation the first action sees (the prologue's bit-exact row), and the policy assignment for P > 1, are those of
 * salp_vec_rollout_policy; a Gaussian policy runs its mean.  The global step grows by `horizon`; salp_stats_t counts only the
 * steps actually taken (env_steps grows by the sum of the records' step increments).  salp_vec_last_launch reports signature
 * 5 with action source 2.  Host pointers: synchronous; device pointers: the call only launches kernels on `stream` (capturable).
 * SALP_ERR_INVALID, with nothing launched and the handle unchanged, for a handle without no_autoreset, num_food_items != 1,
 * free breathing, max_observed_food != 3, a NULL rec or line, horizon < 1, a radius that is not finite and positive, a flag bit
 * other than those two, a device rec (or device line / track) that is not 16-byte aligned, or a policy of another handle. */
enum { SALP_NAV_STEPS = 0, SALP_NAV_STATUS = 1,
       SALP_NAV_PATH = 2, SALP_NAV_LATERAL = 4,                                  /* float64 each */
       SALP_NAV_XMIN = 6, SALP_NAV_XMAX = 8, SALP_NAV_YMIN = 10, SALP_NAV_YMAX = 12,
       SALP_NAV_X = 14, SALP_NAV_Y = 16, SALP_NAV_WORDS = 20 };
enum { SALP_NAV_REACHED = 1, SALP_NAV_COLLIDED = 2, SALP_NAV_CAPTURED = 4 };   /* bits of SALP_NAV_STATUS */
int salp_vec_evaluate_navigation(salp_vec_t* h, const salp_policy_t* pol, int32_t horizon, const double* line,
                                 double goal_radius, void* rec, double* track_or_null, uint32_t flags, void* stream);

/* Current observation of every env without stepping. obs float [n_envs][obs_dim]. */
int salp_vec_observe(salp_vec_t* h, float* obs, uint32_t flags, void* stream);

/* State snapshot (layout above).  f64: double [SALP_F_COUNT(F)][n_envs]; i32: int32
 * [SALP_I_COUNT][n_envs].  set_state ignores the derived ellipse rows and accepts the ranges listed above the info columns
 * ("Ranges accepted by salp_vec_set_state"). */
int salp_vec_get_state(salp_vec_t* h, double* f64, int32_t* i32, uint32_t flags, void* stream);
int salp_vec_set_state(salp_vec_t* h, const double* f64, const int32_t* i32, uint32_t flags,
                       void* stream);

/* Re-keys the draw streams and starts over: afterwards the handle is in exactly the state salp_vec_create(cfg, n, dev,
 * seed, base) returns — new key words, every draw counter at 0, every env freshly reset (snake:133-155 `reset(seed)`,
 * legacy:95-96), statistics and global step cleared; base_num_food_items keeps a value set by
 * salp_vec_set_base_num_food.  Nothing is freed or reallocated and no launch parameter changes (the kernels read the
 * key words from device memory), so device pointers stay valid and a hipGraph captured on this handle before the call
 * replays correctly after it.  Asynchronous on `stream` with device pointers.  obs (may be NULL): float [n_envs][obs_dim],
 * the first observations. */
int salp_vec_reseed(salp_vec_t* h, uint64_t seed, float* obs, uint32_t flags, void* stream);

/* Totals of everything issued so far: waits for the stream of the handle's most recent call (not for the device). */
int salp_vec_get_stats(salp_vec_t* h, salp_stats_t* out);
/* Stream-ordered behind the handle's most recent call; does not synchronise. */
int salp_vec_clear_stats(salp_vec_t* h);
int64_t salp_vec_global_step(const salp_vec_t* h);

/* Which kernel instantiation the handle's most recent step / rollout call ran (introspection for tests and profiles; no
 * reference counterpart): info[0] food slots of the kernel (1, 4, 8, 12, 16), [1] observed-food capacity (3, or 8 = the
 * generic instantiation), [2] 1 = the reference's constants compiled in as literals, [3] forced breathing, [4] the
 * output signature the kernel was compiled for: 1 = obs, reward, terminated, truncated and nothing else, 2 = those four plus
 * final_obs and / or info, 0 = some of the four is NULL (every store tested; always 0 for the generic instantiation's unpacked calls),
 * 3 = the packed record (both halves of a split launch and the generic instantiation too), 4 = the per-env summary record and
 * no per-step output (salp_vec_evaluate_policy: both halves; always with [5] == 2), 5 = the navigation record
 * (salp_vec_evaluate_navigation: both halves, always with [5] == 2), [5] 1 = actions drawn in the kernel,
 * 2 = actions computed by a policy in the kernel (salp_vec_rollout_policy, salp_vec_evaluate_policy), 3 = actions sampled
 * from a Gaussian policy in the kernel (salp_vec_rollout_policy_sampled, salp_vec_evaluate_policy_sampled: separate instantiations),
 * [6] envs served by the unpredicated launch (whole wavefronts), [7] envs served by the predicated launch.
 * [4] is the signature of the kernel that ran: the unpredicated launch's when there was one, else the predicated launch's
 * (predicated kernels exist for signatures 1, 3, 4, 5 and 0 only: a call with final_obs / info runs them as 0). */
int salp_vec_last_launch(const salp_vec_t* h, int64_t info[8]);
/* The output signature of each half of that call: sig[0] the unpredicated launch, sig[1] the predicated launch, -1 for a
 * half that was not launched (or before any call); 4 in each launched half of a salp_vec_evaluate_policy call, 5 of a
 * salp_vec_evaluate_navigation call. */
int salp_vec_last_launch_signatures(const salp_vec_t* h, int64_t sig[2]);
/* What that kernel (the unpredicated one when both were launched) holds per workgroup of 256 threads, from the runtime
 * (hipFuncGetAttributes, hipOccupancyMaxActiveBlocksPerMultiprocessor): info[0] registers per thread (VGPRs), [1] static LDS
 * bytes, [2] scratch (spill) bytes per thread, [3] workgroups resident per CU = wavefronts per SIMD.  The design's occupancy
 * claims (one food >= 4, 4 / 8 slots 4, 12 slots 3, 16 slots 2) are tested against it; no reference counterpart. */
int salp_vec_last_kernel_resources(const salp_vec_t* h, int32_t info[4]);

/* The curriculum's attribute poke `env.base_num_food_items = k` (src/salp/training/continuous_trainer.py:409-411;
 * src/salp/environments/salp_snake_env.py:36): the number of foods placed at every LATER reset of an env
 * (snake:144-148; with random_food_count the upper bound of the draw).  0 <= k <= the num_food_items the
 * handle was created with, which fixes the number of food slots (create with the curriculum's maximum and
 * lower it here).  Takes effect from the next call; envs mid-episode keep their foods. */
int salp_vec_set_base_num_food(salp_vec_t* h, int32_t k);
int32_t salp_vec_base_num_food(const salp_vec_t* h);

#ifdef __cplusplus
}
#endif
#endif /* SALP_VEC_H */
