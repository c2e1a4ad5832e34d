// The K = 3 rollout kernels with 16 food slots and the reference's constants as literals (salp_rollout_kernel.h).
#include "salp_rollout_kernel.h"

RolloutPick salp_rollout_f16_std(bool ragged, bool forced, int sig, int act) { return pick_k3<16, true>(ragged, forced, sig, act); }
