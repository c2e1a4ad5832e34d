// The K = 3 rollout kernels with 1 food slot and the reference's constants as literals (salp_rollout_kernel.h).
#include "salp_rollout_kernel.h"

RolloutPick salp_rollout_f1_std(bool ragged, bool forced, int sig, int act) { return pick_k3<1, true>(ragged, forced, sig, act); }
