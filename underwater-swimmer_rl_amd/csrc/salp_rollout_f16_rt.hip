// The K = 3 rollout kernels with 16 food slots and run-time constants (salp_rollout_kernel.h).
#include "salp_rollout_kernel.h"

RolloutPick salp_rollout_f16_rt(bool ragged, bool forced, int sig, int act) { return pick_k3<16, false>(ragged, forced, sig, act); }
