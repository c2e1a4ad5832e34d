// The K = 3 rollout kernels with 4 food slots and run-time constants (salp_rollout_kernel.h).
#include "salp_rollout_kernel.h"

RolloutPick salp_rollout_f4_rt(bool ragged, bool forced, int sig, int act) { return pick_k3<4, false>(ragged, forced, sig, act); }
