// The K = 3 rollout kernels with 1 food slot and run-time constants (salp_rollout_kernel.h).
#include "salp_rollout_kernel.h"

RolloutPick salp_rollout_f1_rt(bool ragged, bool forced, int sig, int act) { return pick_k3<1, false>(ragged, forced, sig, act); }
