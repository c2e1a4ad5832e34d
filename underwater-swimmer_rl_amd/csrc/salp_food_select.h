// salp_food_select.h — what the two multi-food paths of the rollout kernel share: the result of a selection pass
// (FoodScan), the packed fp64 keys, the lane broadcast of the cooperative placements, and the observation row formed from
// a selection (observe_selected).  The passes that fill a FoodScan are salp_food_reg.h (foods in registers, fp32 keys) and
// salp_food_lds.h (foods in LDS, packed fp64 keys).
#pragma once
#include "salp_device.h"

namespace salp {

constexpr int kFoodLanes = 64;

// Result of one pass over the slots.
//
// Sort keys (salp_food_lds.h: 13..16 slots with K != 3, the <16, 8> generic instantiation; everything else: fp32 keys,
// salp_food_reg.h).  The K nearest are kept by a
// sorted insertion on PACKED keys: the fp64 squared distance with the low 4 bits of its mantissa replaced by the slot
// number (slots are 0..15).  All keys of an env are then distinct, so the compare-exchange of a chain stage is just
// v_min_f64 / v_max_f64 (no index selects) and a smaller key is a nearer food.  The reference orders by sqrt(d2) with a
// stable sort (snake:382): squared distances a few ulp apart can collapse to one distance (then slot order), while
// others inside the 16 ulp of the packing stay distinct (then distance order).  The pass therefore also keeps the
// (K + 1)-th smallest key, and when two consecutive ones of any lane are closer than 2^-44 relative the wavefront
// runs exact_order_lds() — the reference's own key — so the order is the reference's in every case
// (tests/golden/ref_tie_order_f16_k5.npz).  An empty slot's key is kDeadKey | slot (finite, above any distance).
// Everything that leaves the selection (offsets, distance) is recomputed from the slot's exact position.
template <int KMAX>
struct FoodScan {
  double key[KMAX];  // packed keys of the K nearest live foods, ascending               (LDS-food kernels)
  double next;       // the (KMAX + 1)-th smallest packed key                             (LDS-food kernels)
  uint32_t top[KMAX + 1];   // fp32 keys of the K + 1 nearest, ascending                  (register-food kernels)
  bool tie;          // this lane's key order is inside its error bound: the exact order decides
  int idx[KMAX];     // slots of the K nearest, nearest first (-1: none)
  float bx[KMAX], by[KMAX], bd[KMAX];   // offsets and distance of those foods in fp32  (filled by resolve())
  float dsum;        // sum of distances over ALL live foods
};
__device__ __forceinline__ double dead_key() { return __builtin_bit_cast(double, 0x7FEFFFFFFFFFFFF0ull); }
__device__ __forceinline__ double pack_key(double d2, int k) {
  uint2 u = __builtin_bit_cast(uint2, d2);
  u.x = (u.x & ~15u) | (uint32_t)k;                                 // one v_and_or_b32 on the low dword
  return __builtin_bit_cast(double, u);
}
// v_min_f64 / v_max_f64 written as instructions: llvm.minnum on a bit-cast value gets a canonicalising
// v_max_f64 v, v, v in front of it.  Packed keys are never NaN; for min_key(d2, dead) the kernel runs in IEEE
// mode, where the minimum of a quiet NaN (an empty slot) and a number is the number.
__device__ __forceinline__ double min_key(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double min_key_s(double a, double b_uniform) {   // b in an SGPR pair
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(b_uniform));
  return r;
}
__device__ __forceinline__ double max_key(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ int key_slot(double key) { return (int)(__builtin_bit_cast(unsigned long long, key) & 15ull); }
__device__ __forceinline__ bool key_found(double key) { return key < 1.0e300; }

// The observation row from a scan of the CURRENT food set around the CURRENT pose.
// ALLFOUND: every lane shows K live foods (wave-uniform fact established by the caller): no padding selects.
template <int KMAX, bool STD, bool ALLFOUND = false>
__device__ __forceinline__ void observe_selected(const EnvCore& e, const DevParams& P, double rmax, int K, const FoodScan<KMAX>& q,
                                                 int nlive, bool have_rel, float rel0, float (&o)[12 + 4 * KMAX]) {
  SALP_CONSTS;
  o[0] = (float)e.x * (float)CV(inv_W);
  o[1] = (float)e.y * (float)CV(inv_H);
  o[2] = (float)e.vx * 0.2f;
  o[3] = (float)e.vy * 0.2f;
  o[4] = (float)e.th * (float)CV(inv_pi);
  o[5] = (float)e.om * 10.0f;
  o[6] = (float)rmax * (float)CV(inv_R);
  o[7] = (float)bw_phase(e.packed) * 0.5f;
  o[8] = (float)e.water;
  o[9] = (float)e.noz * (float)CV(inv_max_nozzle);
  const float th = (float)e.th;
#pragma unroll
  for (int s = 0; s < KMAX; ++s) {
    float v0 = 0.f, v1 = 0.f, v2 = 1.f, v3 = 0.f;   // padding for an empty slot (snake:412)
    if (s < K) {
      const bool found = ALLFOUND ? true : (q.idx[s] >= 0);
      float rel;
      if (s == 0 && __all(have_rel)) rel = rel0;    // wave-uniform: skips the second atan2
      else {
        rel = relative_heading(q.by[s], q.bx[s], th);
        if (s == 0) rel = have_rel ? rel0 : rel;
      }
      v0 = found ? q.bx[s] * (float)CV(inv_W) : 0.f;
      v1 = found ? q.by[s] * (float)CV(inv_H) : 0.f;
      v2 = found ? q.bd[s] * CV(inv_diag) : 1.f;
      v3 = found ? rel * 0.318309886183791f : 0.f;
    }
    o[10 + 4 * s + 0] = v0; o[10 + 4 * s + 1] = v1; o[10 + 4 * s + 2] = v2; o[10 + 4 * s + 3] = v3;
  }
  const float fcnt = (float)nlive;
  const float s0 = fminf(fcnt * 0.1f, 1.0f);
  const float s1 = (ALLFOUND || nlive > 0) ? (q.dsum * __builtin_amdgcn_rcpf(fcnt)) * CV(inv_diag) : 1.0f;
  if (KMAX == 3) {
    o[22] = s0; o[23] = s1;
  } else {
#pragma unroll
    for (int s = 0; s <= KMAX; ++s) if (s == K) { o[10 + 4 * s] = s0; o[11 + 4 * s] = s1; }
  }
}

// value of `v` in lane `src` (src wave-uniform): two v_readlane instead of two LDS permutes
__device__ __forceinline__ double bcast_lane(double v, int src) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), src);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

}  // namespace salp
