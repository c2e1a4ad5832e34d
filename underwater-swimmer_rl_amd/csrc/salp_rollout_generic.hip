// The generic-K rollout kernels (K != 3: run-time constants, K <= 8): 12 slots — up to 12 foods, the register-food form,
// 2 wavefronts per SIMD, not 1 — and 16; the packed signature, else kSigPartial for every output; actions are read.
#include "salp_rollout_kernel.h"

namespace {
template <int FMAX>
RolloutPick pick_generic(bool ragged, bool forced, int sig) {
  if (sig == kSigPacked)
    return ragged ? (forced ? picked<FMAX, 8, true, false, kSigPacked, true, ACT_READ>() : picked<FMAX, 8, false, false, kSigPacked, true, ACT_READ>())
                  : (forced ? picked<FMAX, 8, true, false, kSigPacked, false, ACT_READ>() : picked<FMAX, 8, false, false, kSigPacked, false, ACT_READ>());
  return ragged ? (forced ? picked<FMAX, 8, true, false, kSigPartial, true, ACT_READ>() : picked<FMAX, 8, false, false, kSigPartial, true, ACT_READ>())
                : (forced ? picked<FMAX, 8, true, false, kSigPartial, false, ACT_READ>() : picked<FMAX, 8, false, false, kSigPartial, false, ACT_READ>());
}
}  // namespace

RolloutPick salp_rollout_generic12(bool ragged, bool forced, int sig, int) { return pick_generic<12>(ragged, forced, sig); }
RolloutPick salp_rollout_generic16(bool ragged, bool forced, int sig, int) { return pick_generic<16>(ragged, forced, sig); }
