// salp_snake_math_probe.h — test support: the snake step's math primitives on their own.  salp_snake_math_probe
// (salp_vec.hip; its kernel is in salp_service_kernels.h) runs one of sincos_small_t / sin_nozzle_t / atan2_fast /
// cos_wrapped / relative_heading (salp_snake_math.h), philox4x32_10 / u53 (salp_philox.h) or jet_thrust_terms (salp_step.h)
// on the device, element i on thread i of 256-thread blocks, compiled with the flags of the rollout units.  The references
// are in tests/snake_math_cases.py (the host twin of sincos_small, mpmath, a Python emulation in the kernel's operation
// order); tests/test_gpu_snake_math.py holds the device to them.  Not part of the public ABI (include/salp_vec.h).
//
// Rows are [n] doubles; fp32 and uint32 values travel exactly inside doubles.
//   function                     in                                             out
//   SINCOS_T                     x                                              s, c
//   SIN_NOZZLE_T                 x                                              sin x
//   ATAN2 / ATAN2_PRECISE        y, x (fp32)                                    angle (fp32)
//   COS_WRAPPED                  x (fp32)                                       cos x (fp32)
//   REL_HEADING / _PRECISE       dy, dx, th (fp32)                              wrapped heading (fp32)
//   PHILOX                       c0, c1, c2, c3, k0, k1 (uint32)                four words (uint32)
//   U53                          hi, lo (uint32)                                the uniform
//   THRUST_STD / THRUST_RT       th, noz, water, r, rng, genv_lo, genv_hi       ax, ay, bx, by, cx, cy, om (ThrustTerms)
// THRUST_*: jet_thrust_terms<true> / <false> with the DevParams that make_params derives from `cfg` (NULL: the defaults)
// and the key words of `seed`; THRUST_STD is refused for a config whose constants are not the literals (is_std).
#pragma once
#include <stdint.h>

#include "../../include/salp_vec.h"   // salp_config_t

enum {
  SALP_SNAKE_MATH_SINCOS_T = 0, SALP_SNAKE_MATH_SIN_NOZZLE_T = 1, SALP_SNAKE_MATH_ATAN2 = 2, SALP_SNAKE_MATH_ATAN2_PRECISE = 3,
  SALP_SNAKE_MATH_COS_WRAPPED = 4, SALP_SNAKE_MATH_REL_HEADING = 5, SALP_SNAKE_MATH_REL_HEADING_PRECISE = 6,
  SALP_SNAKE_MATH_PHILOX = 7, SALP_SNAKE_MATH_U53 = 8, SALP_SNAKE_MATH_THRUST_STD = 9, SALP_SNAKE_MATH_THRUST_RT = 10
};
// `in` / `out` are host arrays.  0 on success, negative with salp_last_error() set: -1 for a NULL array, n outside
// [1, 2^24], an unknown code or a config that is refused (nothing is launched), -2 for a device that is absent.
extern "C" int salp_snake_math_probe(int device_id, int function, const salp_config_t* cfg, uint64_t seed, const double* in,
                                     double* out, int64_t n);
