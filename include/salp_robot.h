/*
 * salp_robot.h — C ABI of the batched HEAD simulator: the reference's jet-propelled
 * rigid-body `Robot` (src/salp/environments/robot.py) under `SalpRobotEnv`
 * (src/salp/environments/salp_robot_env.py), one robot per GPU lane.
 *
 *   salp_robot_config_default   Robot.__init__ / Nozzle.__init__ arguments of train_robot.py:12-18,
 *                               SalpRobotEnv.__init__ (salp_robot_env.py:32-37)
 *   salp_robot_vec_create       make_env() (train_robot.py:10-22) x n_envs
 *   salp_robot_vec_reset        SalpRobotEnv.reset            salp_robot_env.py:98-128
 *   salp_robot_vec_step         SalpRobotEnv.step             salp_robot_env.py:139-201 — ONE env step is one
 *                               whole breathing cycle: Robot.set_control + step_through_cycle
 *                               (robot.py:335-358, 422-445), up to ~1450 Euler steps of dt = 0.01 s
 *   salp_robot_vec_step_history  the same step, plus the per-Euler-step history that step_through_cycle
 *                               collects with Robot.get_current_values (robot.py:398-445) for a range of envs
 *   salp_robot_vec_history_capacity  samples per env that salp_robot_vec_step_history may write
 *   salp_robot_vec_trajectory   compare_actions_with_states (compare_trajectories.py:19-117) for every robot of the
 *                               handle at once, each with its own physical parameters (system identification)
 * (H cycles per robot in one launch, open loop or under an in-kernel policy: salp_robot_rollout.h.)
 *
 * Actions are float32 [n][3] in the env's Box ([0,1], [0,1], [-1,1]): contraction / 0.06 m, coast time
 * / 10 s, nozzle yaw / (pi/2).  They are widened to fp64 before the rescale of salp_robot_env.py:129-137.
 * The reference does not clip them, and neither does this library, with one exception: the length of a
 * breathing cycle (refill + jet + coast, 14.5 s at most inside the Box) is cut at 14.6 s, and a non-finite
 * length runs no Euler step — one out-of-Box or inf action must not spin a wavefront of 64 robots for ever
 * (the reference would stall that one CPU env for the corresponding number of Euler steps).
 * Observation float32 [n][6]: x - target_x, y - target_y, body-frame vx, vy, yaw, yaw rate (:400-420).
 * Same conventions as salp_vec.h (status codes, SALP_DEVICE_PTRS, streams, same-step autoreset).
 * The target point of each episode (np.random.uniform, :247-250) comes from
 *   Philox4x32-10(counter = (env_lo, env_hi, episode#, 16), key = seed): x from u53(w0,w1), y from u53(w2,w3).
 *
 * Cycle history (salp_robot_vec_step_history).  The reference's env step fills one history per Euler step
 * (`[initial] + one per step`) and returns it in `info` (salp_robot_env.py:194-198).  Here it is recorded for the
 * envs [hist_begin, hist_begin + hist_count) only, as float32 [hist_count][capacity][SALP_H_COUNT]:
 *   - samples: for an env whose cycle ran T Euler steps, sample 0 is the state at the cycle start (after
 *     set_control) and sample k the state after Euler step k; with stride s the samples are at steps
 *     0, s, 2s, ... plus step T whenever T % s != 0, so the record always ends on the state the observation
 *     reports.  history_len[j] = number of samples of env hist_begin + j (T + 1 at stride 1); samples past it
 *     are not written.
 *   - channels SALP_H_*: position xyz, body-frame velocity, Euler angles (roll, pitch, yaw), angular velocity,
 *     length, width, phase (0 REFILL / 1 JET / 2 COAST / 3 REST, robot.py:194) and the rescaled nozzle yaw
 *     (constant over a cycle).  These are what the env info, the renderer and compare_trajectories read; the
 *     reference's other histories (acceleration, Euler-angle rate, jet / drag forces and torques, area, volume,
 *     mass, drag coefficient) have no consumer and are not recorded.
 *   - an env that terminates or truncates reports the cycle that just ran, before its autoreset.
 *   - known difference: sample 0 has the init shape and REST in length / width / phase; the reference carries
 *     the previous cycle's last values, which differ only when that cycle's last Euler step landed exactly on
 *     a phase boundary, and then by <= 1 ulp in the shape.
 *   - capacity must be >= salp_robot_vec_history_capacity(h, stride) (= the longest cycle the 14.6 s cut allows
 *     at the configured dt, in samples; -1 if that cycle exceeds 2^24 Euler steps, a dt the history calls refuse).
 *     stride < 1, a range outside [0, n), a smaller capacity or a NULL history with hist_count > 0 return -1 and
 *     launch nothing; hist_count == 0 is salp_robot_vec_step.
 *   - with SALP_DEVICE_PTRS history must be 16-byte aligned, nothing is allocated (graph-capturable), and nothing
 *     past history_len[j] is written.  Host pointers are staged like the other outputs: the device buffer is
 *     hist_count * capacity * 64 bytes, and hist_count rows of the call's longest record are copied back (in rows
 *     with a shorter record the samples past history_len are overwritten with unspecified values).
 *
 * Trajectory comparison (salp_robot_vec_trajectory).  Robot i of the handle runs what compare_actions_with_states
 * does with one Robot: Robot.reset (robot.py:287-333: origin, zero velocities and angles, rest shape, cycle time 0),
 * then for t in [0, cycles) nozzle.set_yaw_angle + solve_angles + set_control + step_through_cycle with actions[t]
 * (compare_trajectories.py:51-72), and reports states[t][i] = position x, y, body-frame velocity x, y, yaw, yaw rate.
 *   - the call neither reads nor writes the env state of the handle (SALP_R_* rows, target draws, schedule): a
 *     later salp_robot_vec_step behaves as if it never happened.
 *   - actions are fp64 in the reference's units: contraction (m), coast time (s), nozzle yaw (rad), not the env's Box;
 *     no rescale.  [cycles][3], shared by every robot; with SALP_ROBOT_PER_ROBOT_ACTIONS [cycles][n_envs][3] (run in
 *     index order, no longest-cycle-first schedule).  The cycle-length guard of the env step applies: a cycle longer
 *     than 14.6 s is cut there, and a non-finite length runs no Euler step.
 *   - params (nullable) double [SALP_RP_COUNT][n_envs]: robot i takes column i for what the reference takes from
 *     Robot(...), Nozzle(...), set_environment(density) and _drag_coefficents; dt, the tank, max_cycles and the
 *     contract / release rates stay the handle's (nozzle_length3 is drawing code only).  NULL = the handle's config
 *     for every robot, bit-identical to a table filled with it.  The table is not validated (it may live on the
 *     device): a zero, negative or NaN entry gives that robot meaningless or non-finite output and nothing else;
 *     cycle lengths depend only on the actions and dt, and other robots move by no more than the wave-uniform exact
 *     sin / cos and sqrt fallbacks couple lanes (< 1e-12 relative per cycle).
 *   - expected (nullable) double [cycles][6]; metrics double [n_envs][SALP_RM_COUNT] needs it: the means over t of
 *     |d(x, y)|, |d(vx, vy)|, |d yaw| (not wrapped), |d yaw rate| and the max over t of |d(x, y)|
 *     (compare_trajectories.py:77-86), summed in fp64 in cycle order; a NaN error gives a NaN mean and max.
 *   - states double [cycles][n_envs][6], metrics, inner_steps int32 [cycles][n_envs] (Euler steps per cycle,
 *     len(position_history) - 1) are each nullable; a metrics-only call writes no per-cycle data.
 *   - -1 and no launch: NULL handle or actions, cycles outside [1, SALP_ROBOT_MAX_TRAJECTORY_CYCLES], unknown flag
 *     bits, metrics without expected, a dt the history calls refuse.  The cap bounds one launch on a shared GPU.
 *   - SALP_DEVICE_PTRS: nothing is allocated or synchronised (graph-capturable); host pointers are staged and copied
 *     back, and the call returns after the stream is synchronised.
 */
#ifndef SALP_ROBOT_H
#define SALP_ROBOT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct salp_robot_config {
  uint32_t struct_size;
  int32_t width, height;          /* 900, 700 (salp_robot_env.py:32) */
  double tank_margin;             /* 50 */
  /* Robot(dry_mass, init_length, init_width, max_contraction, nozzle), train_robot.py:14-15 */
  double dry_mass;                /* 1.0 kg */
  double init_length;             /* 0.3 m */
  double init_width;              /* 0.15 m */
  double max_contraction;         /* 0.06 m */
  double density;                 /* 1000 kg/m^3 (set_environment) */
  double dt;                      /* 0.01 s (robot.py:214) */
  double drag_coefficient_min;    /* 0.4 (robot.py:222) */
  double drag_coefficient_max;    /* 1.0 */
  /* Nozzle(length1, length2, length3, area, mass), train_robot.py:12 */
  double nozzle_length1, nozzle_length2, nozzle_length3;   /* 0.05 each */
  double nozzle_area;             /* 0.00016 m^2 */
  double nozzle_mass;             /* 1.0 kg */
  double nozzle_gamma;            /* pi/4 (robot.py:31) */
  int32_t max_cycles;             /* 500 (salp_robot_env.py:183) */
  int32_t reserved0;
} salp_robot_config_t;

/* rows of the fp64 state snapshot [SALP_R_COUNT][n_envs] */
enum {
  SALP_R_POS = 0, SALP_R_VEL = 3, SALP_R_EULER = 6, SALP_R_OMEGA = 9, SALP_R_VEL_WORLD = 12, SALP_R_PREV_I = 15,
  SALP_R_TARGET = 18, SALP_R_PREV_DIST = 20, SALP_R_VOLUME = 21, SALP_R_ANGLE1 = 22, SALP_R_ANGLE2 = 23,
  SALP_R_TIME = 24, SALP_R_CYCLE = 25, SALP_R_RNG = 26, SALP_R_COUNT = 27
};
/* channels of one float32 cycle-history sample [SALP_H_COUNT] (salp_robot_vec_step_history) */
enum {
  SALP_H_POS = 0, SALP_H_VEL = 3, SALP_H_EULER = 6, SALP_H_OMEGA = 9, SALP_H_LENGTH = 12, SALP_H_WIDTH = 13,
  SALP_H_STATE = 14, SALP_H_NOZZLE_YAW = 15, SALP_H_COUNT = 16
};

/* rows of the per-robot parameter table double [SALP_RP_COUNT][n_envs] (salp_robot_vec_trajectory); the names are
 * those of the salp_robot_config_t fields */
enum {
  SALP_RP_DRY_MASS = 0, SALP_RP_INIT_LENGTH = 1, SALP_RP_INIT_WIDTH = 2, SALP_RP_MAX_CONTRACTION = 3, SALP_RP_DENSITY = 4,
  SALP_RP_DRAG_COEFFICIENT_MIN = 5, SALP_RP_DRAG_COEFFICIENT_MAX = 6, SALP_RP_NOZZLE_LENGTH1 = 7,
  SALP_RP_NOZZLE_LENGTH2 = 8, SALP_RP_NOZZLE_AREA = 9, SALP_RP_NOZZLE_MASS = 10, SALP_RP_NOZZLE_GAMMA = 11,
  SALP_RP_COUNT = 12
};
/* columns of the per-robot metrics double [n_envs][SALP_RM_COUNT] (salp_robot_vec_trajectory) */
enum {
  SALP_RM_POSITION_ERROR = 0, SALP_RM_VELOCITY_ERROR = 1, SALP_RM_ANGLE_ERROR = 2, SALP_RM_MAX_POSITION_ERROR = 3,
  SALP_RM_ANGULAR_VELOCITY_ERROR = 4, SALP_RM_COUNT = 5
};
/* flag bit of salp_robot_vec_trajectory next to SALP_DEVICE_PTRS (1u): actions are [cycles][n_envs][3] */
enum { SALP_ROBOT_PER_ROBOT_ACTIONS = 2u };
enum { SALP_ROBOT_MAX_TRAJECTORY_CYCLES = 1024 };

typedef struct salp_robot_vec salp_robot_vec_t;

const char* salp_robot_last_error(void);   /* message of the calling thread's last failed salp_robot_* call */
int salp_robot_config_default(salp_robot_config_t* cfg);
int salp_robot_vec_create(const salp_robot_config_t* cfg, int64_t n_envs, int device_id, uint64_t seed,
                          int64_t env_index_base, salp_robot_vec_t** out);
void salp_robot_vec_destroy(salp_robot_vec_t* h);
int64_t salp_robot_vec_num_envs(const salp_robot_vec_t* h);
int salp_robot_vec_reset(salp_robot_vec_t* h, const uint8_t* mask, float* obs, uint32_t flags, void* stream);
/* obs float [n][6]; reward float [n]; terminated/truncated uint8 [n]; final_obs (nullable) float [n][6]
 * rows of finished envs; inner_steps (nullable) int32 [n] = Euler steps of this cycle. */
int salp_robot_vec_step(salp_robot_vec_t* h, const float* act, float* obs, float* reward, uint8_t* terminated,
                        uint8_t* truncated, float* final_obs, int32_t* inner_steps, uint32_t flags, void* stream);
int salp_robot_vec_get_state(salp_robot_vec_t* h, double* state, uint32_t flags, void* stream);
/* most samples per env one salp_robot_vec_step_history call writes at this stride (-1 if h is NULL or stride < 1) */
int32_t salp_robot_vec_history_capacity(const salp_robot_vec_t* h, int32_t stride);
/* salp_robot_vec_step plus the cycle history of envs [hist_begin, hist_begin + hist_count): history float
 * [hist_count][capacity][SALP_H_COUNT], history_len (nullable) int32 [hist_count] (see the top of this file) */
int salp_robot_vec_step_history(salp_robot_vec_t* h, const float* act, float* obs, float* reward, uint8_t* terminated,
                                uint8_t* truncated, float* final_obs, int32_t* inner_steps, int64_t hist_begin,
                                int64_t hist_count, int32_t stride, int32_t capacity, float* history,
                                int32_t* history_len, uint32_t flags, void* stream);
/* compare_actions_with_states for every robot, each with its own parameters (see the top of this file): params
 * (nullable) double [SALP_RP_COUNT][n], actions double [cycles][3] or [cycles][n][3], expected (nullable) double
 * [cycles][6], states (nullable) double [cycles][n][6], metrics (nullable) double [n][SALP_RM_COUNT], inner_steps
 * (nullable) int32 [cycles][n] */
int salp_robot_vec_trajectory(salp_robot_vec_t* h, const double* params, const double* actions, int32_t cycles,
                              const double* expected, double* states, double* metrics, int32_t* inner_steps,
                              uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
