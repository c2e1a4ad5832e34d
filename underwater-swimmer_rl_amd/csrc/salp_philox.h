// salp_philox.h — Philox4x32-10 and the 53-bit uniform of the draw streams (include/salp_vec.h "Randomness",
// include/salp_robot.h).  Shared by the snake simulator and the robot simulator; includes nothing of either.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace salp {

// ------------------------------------------------------------------ Philox4x32-10
struct U4 { uint32_t x, y, z, w; };
// (gfx950 has no v_xor3_b32: the two xors per word stay two instructions.)
__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                            uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}
__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {
  // ((hi>>5)*2^26 + (lo>>6)) / 2^53 : every operation is exact
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) * 1.1102230246251565e-16;
}

}  // namespace salp
