// robot_params_host.cpp — host twin of the robot simulator's parameter derivation and argument checks (TEST
// INFRASTRUCTURE).  Compiles csrc/salp_robot_params.h as plain C++ (oracle/Makefile, the flags of the math twin) and
// exports what salp_robot_vec_create, salp_robot_vec_step_history and salp_robot_vec_trajectory decide before they touch
// a GPU: the default config, create's refusals, the launch parameters of a config, the longest cycle in Euler steps and
// the history capacity, the refusals of the history and trajectory calls, the schedule's bin of an action, and the list
// of physical parameters itself.
#include "../underwater-swimmer_rl_amd/csrc/salp_robot_params.h"

namespace {
struct PhysRow { const char* field; const char* row; const char* member; int row_value; double (*value)(const RobotParams&); };
#define SALP_ROBOT_PHYS_TWIN(field, row, member) {#field, #row, #member, (int)row, [](const RobotParams& P) { return P.member; }},
const PhysRow kPhys[] = {SALP_ROBOT_PHYS(SALP_ROBOT_PHYS_TWIN)};
#undef SALP_ROBOT_PHYS_TWIN
constexpr int kPhysCount = (int)(sizeof(kPhys) / sizeof(kPhys[0]));
constexpr int kDerivedCount = 11;   // dt, x_min, x_span, y_min, y_span, max_cycles, seed_lo, seed_hi, env_base, n, pitch
}  // namespace

extern "C" {

int salp_robot_params_host_config_sizeof(void) { return (int)sizeof(salp_robot_config_t); }
void salp_robot_params_host_default(salp_robot_config_t* c) { robot_config_default(c); }

// The status of check_robot_create(); *why (nullable) gets the message, "" when the arguments are accepted.
int salp_robot_params_host_check_create(const salp_robot_config_t* c, int64_t n_envs, int64_t base, const char** why) {
  const char* msg = "";
  const int rc = check_robot_create(c, n_envs, base, &msg);
  if (why) *why = msg;
  return rc;
}

// The list SALP_ROBOT_PHYS: row i's config field, SALP_RP_* name, RobotParams member, and the value of the SALP_RP_* name
int salp_robot_params_host_phys_count(void) { return kPhysCount; }
const char* salp_robot_params_host_phys_field(int i) { return kPhys[i].field; }
const char* salp_robot_params_host_phys_row(int i) { return kPhys[i].row; }
const char* salp_robot_params_host_phys_member(int i) { return kPhys[i].member; }
int salp_robot_params_host_phys_row_value(int i) { return kPhys[i].row_value; }

// make_robot_params() as salp_robot_params_host_make_count() doubles: the members of the list in list order, then dt,
// x_min, x_span, y_min, y_span, max_cycles, seed_lo, seed_hi, env_base, n, pitch (each exact in a double for the
// values the tests use)
int salp_robot_params_host_make_count(void) { return kPhysCount + kDerivedCount; }
void salp_robot_params_host_make(const salp_robot_config_t* c, int64_t n_envs, uint64_t seed, int64_t base, double* out) {
  const RobotParams P = make_robot_params(*c, n_envs, seed, base);
  for (int i = 0; i < kPhysCount; ++i) out[i] = kPhys[i].value(P);
  const double derived[kDerivedCount] = {P.dt, P.x_min, P.x_span, P.y_min, P.y_span, (double)P.max_cycles, (double)P.seed_lo,
                                         (double)P.seed_hi, (double)P.env_base, (double)P.n, (double)P.pitch};
  for (int i = 0; i < kDerivedCount; ++i) out[kPhysCount + i] = derived[i];
}

// kPi, kActContraction, kActCoast, kActYaw, kContractRate, kReleaseRate, kMaxCycleTime, kSchedBins, kMaxHistorySteps
void salp_robot_params_host_constants(double out[9]) {
  const double v[9] = {kPi, kActContraction, kActCoast, kActYaw, kContractRate, kReleaseRate, kMaxCycleTime, (double)kSchedBins,
                       (double)kMaxHistorySteps};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
}

int64_t salp_robot_params_host_max_steps(double dt) { return robot_max_steps(dt); }
int64_t salp_robot_params_host_history_capacity(int64_t max_steps, int32_t stride) { return history_capacity(max_steps, stride); }

// The status of check_history_args(); the message goes to msg (msg_size bytes), "" when accepted; *plain_step (nullable)
// is 1 when the range is empty.  `history` is only compared with NULL and tested for alignment, never read.
int salp_robot_params_host_check_history(int64_t n, int64_t max_steps, int64_t hist_begin, int64_t hist_count, int32_t stride,
                                         int32_t capacity, const void* history, uint32_t flags, int* plain_step, char* msg,
                                         int msg_size) {
  if (msg_size > 0) msg[0] = 0;
  bool plain = false;
  const int rc = check_history_args(n, max_steps, hist_begin, hist_count, stride, capacity, history, flags, &plain, msg,
                                    (size_t)msg_size);
  if (plain_step) *plain_step = plain ? 1 : 0;
  return rc;
}

// The status of check_trajectory_args(); the message goes to msg (msg_size bytes), "" when accepted.
int salp_robot_params_host_check_trajectory(int64_t max_steps, int32_t cycles, uint32_t flags, int has_expected, int has_metrics,
                                            char* msg, int msg_size) {
  if (msg_size > 0) msg[0] = 0;
  return check_trajectory_args(max_steps, cycles, flags, has_expected != 0, has_metrics != 0, msg, (size_t)msg_size);
}
int salp_robot_params_host_max_trajectory_cycles(void) { return SALP_ROBOT_MAX_TRAJECTORY_CYCLES; }

// schedule_bin() of n actions: act float [n][3] as the step takes them (the third component is not read)
void salp_robot_params_host_schedule_bins(const float* act, int64_t n, int32_t* bins) {
  for (int64_t i = 0; i < n; ++i) bins[i] = schedule_bin(act[i * 3 + 0], act[i * 3 + 1]);
}

}  // extern "C"
