// salp_snake_math.h — the fp64 and fp32 math of the snake step that has no state in it: Python's max / min, the thrust
// block's constant table with sincos_small_t / sin_nozzle_t on it, and the fp32 helpers of the observation and the reward
// (atan2_fast, cos_wrapped, relative_heading).  Device code only; the numerics contract is in salp_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace salp {

__device__ __forceinline__ double pymax(double a, double b) { return (b > a) ? b : a; }
__device__ __forceinline__ double pymin(double a, double b) { return (b < a) ? b : a; }
__device__ __forceinline__ bool is_none(double fx) { return fx != fx; }

#define SALP_PI 3.141592653589793
#define SALP_2PI 6.283185307179586
#define SALP_PIO2 1.5707963267948966

// ------------------------------------------------------------------ fp64 trigonometry
// sincos_small (Cody-Waite reduction by pi/2, fdlibm kernel polynomials) lives in salp_fp64_math.h with the other
// hand-written fp64 routines that have a host twin and an error bound of their own under test.

// ---- thrust-block constants through the scalar cache ------------------------------------------------
// gfx950 has no 64-bit literals: every fp64 constant of a kernel is an s_mov_b32 pair (or a v_mov_b32 pair
// when it is the addend of a v_fmac_f64), and the wavefront issues ONE instruction of any kind per 4 cycles
// (SQ counters, profiles/r02/ab_notes.md): in the 12-food kernel ~250 of ~1200 instructions per step were
// such moves, 99 of them in the thrust block.  The constants of the thrust block therefore sit in a table in
// constant memory and are fetched with scalar loads — one s_load_dwordx8/x16 brings 4 / 8 of them into SGPRs,
// which v_fma_f64 / v_mul_f64 take directly as an operand.  The table pointer is made opaque at the point of
// use so that the loads stay inside the (conditional) thrust block instead of being hoisted across the step
// loop, where they would only be spilled.  Values and evaluation order are those of sincos_small
// (salp_fp64_math.h) and of sin_nozzle_t's polynomial below: results are bit-identical (tests/test_gpu_snake_math.py holds
// sincos_small_t to sincos_small's host twin bit for bit; tests/test_snake_math.py holds every row to its definition).
typedef const double __attribute__((address_space(4))) tbl_double;
enum {
  TT_2OPI = 0, TT_PIO2_1, TT_PIO2_1T, TT_S5, TT_S4, TT_S3, TT_S2, TT_S1,          // sincos reduction, sin kernel
  TT_S0, TT_C6, TT_C5, TT_C4, TT_C3, TT_C2, TT_C1, TT_PAD0,                        // cos kernel
  TT_N10, TT_N9, TT_N8, TT_N7, TT_N6, TT_N5, TT_N4, TT_N3,                         // sin_nozzle_t
  TT_N2, TT_N1, TT_K012, TT_K0002, TT_K07, TT_K00005, TT_K00003, TT_PIO2,          // thrust scalings
  TT_DL, TT_K03, TT_K008, TT_K005, TT_J_S3, TT_J_S2, TT_J_S1, TT_J_S0,             // side thrust, jitter sin
  TT_J_C3, TT_J_C2, TT_J_C1, TT_K004, TT_K0002J, TT_K04, TT_COUNT
};
__constant__ double kThrustTbl[TT_COUNT + 2] = {
  6.36619772367581382433e-01, 1.57079632673412561417e+00, 6.07710050650619224932e-11,
  1.58969099521155010221e-10, -2.50507602534068634195e-08, 2.75573137070700676789e-06, -1.98412698298579493134e-04,
  8.33333333332248946124e-03,
  -1.66666666666666324348e-01, -1.13596475577881948265e-11, 2.08757232129817482790e-09, -2.75573143513906633035e-07,
  2.48015872894767294178e-05, -1.38888888888741095749e-03, 4.16666666666666019037e-02, 0.0,
  1.9572941063391263e-20, -8.2206352466243295e-18, 2.8114572543455206e-15, -7.6471637318198164e-13,
  1.6059043836821613e-10, -2.5052108385441720e-08, 2.7557319223985893e-06, -1.9841269841269841e-04,
  8.3333333333333332e-03, -1.6666666666666666e-01, 0.012, 0.0002, 0.7, 0.00005, 0.00003, 1.5707963267948966,
  -6.123233995736766e-17, 0.3, 0.008, 0.05, 2.7557319223985893e-06, -1.9841269841269841e-04, 8.3333333333333332e-03,
  -1.6666666666666666e-01,
  2.4801587301587302e-05, -1.3888888888888889e-03, 4.1666666666666664e-02, 0.04, 0.002, 0.4, 0.0, 0.0
};
__device__ __forceinline__ tbl_double* thrust_table() {
  tbl_double* t = (tbl_double*)kThrustTbl;
  asm volatile("" : "+s"(t));
  return t;
}
// a * b + c and a * c with the constant c in an SGPR pair, written as instructions: left to itself the
// compiler copies a scalar addend into VGPRs (two v_mov_b32) to use the two-address v_fmac_f64.
__device__ __forceinline__ double fma_s(double a, double b, double c_uniform) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c_uniform));
  return r;
}
__device__ __forceinline__ double mul_s(double a, double c_uniform) {
  double r;
  asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(c_uniform));
  return r;
}
__device__ __forceinline__ void sincos_small_t(tbl_double* T, double x, double& s, double& c) {
  const double fn = __builtin_rint(mul_s(x, T[TT_2OPI]));
  const double nfn = -fn;
  double r = fma(nfn, T[TT_PIO2_1], x);
  r = fma(nfn, T[TT_PIO2_1T], r);
  const double z = r * r;
  double ps = fma_s(z, (double)T[TT_S5], T[TT_S4]);
  ps = fma_s(z, ps, T[TT_S3]);
  ps = fma_s(z, ps, T[TT_S2]);
  ps = fma_s(z, ps, T[TT_S1]);
  const double v = z * r;
  const double sr = fma(v, fma_s(z, ps, T[TT_S0]), r);
  double pc = fma_s(z, (double)T[TT_C6], T[TT_C5]);
  pc = fma_s(z, pc, T[TT_C4]);
  pc = fma_s(z, pc, T[TT_C3]);
  pc = fma_s(z, pc, T[TT_C2]);
  pc = fma_s(z, pc, T[TT_C1]);
  const double hz = 0.5 * z;
  const double w = 1.0 - hz;
  const double cr = w + (((1.0 - w) - hz) + z * (z * pc));
  const int q = (int)fn & 3;
  const double s0 = (q & 1) ? cr : sr;
  const double c0 = (q & 1) ? sr : cr;
  s = (q & 2) ? -s0 : s0;
  c = ((q + 1) & 2) ? -c0 : c0;
}
// sin(x) for |x| <= pi/3 (the nozzle angle): odd Taylor polynomial to x^21.  The polynomial's truncation error is < 2e-22
// for |x| <= pi/3; the function's error is its roundings, <= 1 ulp of sin x (the last fma rounds x + x z p once, the
// correction is <= 0.19 |x| with a few ulps of relative error; measured 0.95 ulp, tests/test_snake_math.py).  The
// coefficients (1/21!, -1/19!, ... -1/3!) are rows TT_N10 .. TT_N1 of the table.  The sum of -0 and the correction's +0
// is +0, so the sign of a zero argument is copied over: sin(-0) = -0, as the reference's.
__device__ __forceinline__ double sin_nozzle_t(tbl_double* T, double x) {
  const double z = x * x;
  double p = fma_s(z, (double)T[TT_N10], T[TT_N9]);
  p = fma_s(z, p, T[TT_N8]);
  p = fma_s(z, p, T[TT_N7]);
  p = fma_s(z, p, T[TT_N6]);
  p = fma_s(z, p, T[TT_N5]);
  p = fma_s(z, p, T[TT_N4]);
  p = fma_s(z, p, T[TT_N3]);
  p = fma_s(z, p, T[TT_N2]);
  p = fma_s(z, p, T[TT_N1]);
  return __builtin_copysign(fma(x * z, p, x), x);
}

// fp32 helpers for quantities that only leave the simulator (observation angle, reward shaping).  Three food bearings per
// step were 110 of the 12-food kernel's ~590 VALU instructions per wavefront-step (round 2: degree-17 polynomial, Newton
// step on the reciprocal, compare / select unfolding and wrapping); the contract is 1e-5 on angle / pi.
// atan2 for the food bearing: t = min / max through v_rcp_f32 (1 ulp), odd minimax polynomial on [0, 1] (Remez fits),
// octant / quadrant unfolding, sign by bit copy.  PRECISE = false (bearings that only go to the observation): degree 11.
// PRECISE = true (the nearest food's bearing, which the reward multiplies by proximity_reward_weight, 5 in
// single_food.yaml): degree 13.  Two errors, not one:
//   polynomial (the fit's own, in exact arithmetic)       1.7e-6 rad (degree 11)    2.5e-7 rad (degree 13)
//   function (with the fp32 roundings of t, the Horner steps, t p and the unfolding subtractions from pi/2 and pi, whose
//   results carry up to 1.2e-7 of rounding each, and pi_f32 - pi = 8.7e-8; correctly rounded reciprocal)
//                                                         1.9e-6 rad = 6.1e-7 of pi  5.0e-7 .. 5.4e-7 rad
// v_rcp_f32 adds one ulp of t (<= 1.2e-7 rad).  The device's measured figures are in DESIGN.md §4; tests/test_gpu_snake_math.py
// asserts the function's error, never the polynomial's.  Both arguments under the 1e-30 floor: t = min * 1e30, not atan2
// (an fp64 tank position yields offsets that are 0 or above 1e-14).
template <bool PRECISE>
__device__ __forceinline__ float atan2_fast(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = __builtin_fmaxf(__builtin_fmaxf(ax, ay), 1.0e-30f);   // v_max3_f32; atan2(0, 0) = 0 (math.atan2): t = 0 * 1e30
  const float mn = __builtin_fminf(ax, ay);
  const float t = mn * __builtin_amdgcn_rcpf(mx);
  const float z = t * t;
  float p;
  if (PRECISE) {
    p = fmaf(z, 0.006811792962253094f, -0.0336042195558548f);
    p = fmaf(z, p, 0.07962366938591003f);
    p = fmaf(z, p, -0.1323334276676178f);
    p = fmaf(z, p, 0.19807815551757812f);
    p = fmaf(z, p, -0.3331736922264099f);
    p = fmaf(z, p, 0.9999961256980896f);
  } else {
    p = fmaf(z, -0.01171913556754589f, 0.05264735221862793f);
    p = fmaf(z, p, -0.116426482796669f);
    p = fmaf(z, p, 0.19354037940502167f);
    p = fmaf(z, p, -0.33262282609939575f);
    p = fmaf(z, p, 0.9999772310256958f);
  }
  float a = t * p;
  if (ay > ax) a = 1.57079632679489662f - a;
  if (x < 0.0f) a = 3.14159265358979324f - a;
  return __builtin_copysignf(a, y);
}

// cos(x) for |x| <= pi (a wrapped heading): fold to [0, pi/2], even Taylor polynomial to x^12.  The polynomial's truncation
// error is 6.5e-9; the function's error is 1.6e-7: the fold pi_f32 - |x| is off by pi_f32 - pi = 8.7e-8 where the slope is 1,
// and the result is rounded to fp32 (3e-8 .. 6e-8).  No reciprocal: the device equals the fp32 emulation bit for bit.
__device__ __forceinline__ float cos_wrapped(float x) {
  float ax = fabsf(x);
  const bool flip = ax > 1.57079632679489662f;
  if (flip) ax = 3.14159265358979324f - ax;
  const float z = ax * ax;
  float p = fmaf(z, 2.08767569878681e-09f, -2.755731922398589e-07f);
  p = fmaf(z, p, 2.48015873015873e-05f);
  p = fmaf(z, p, -1.3888888888888889e-03f);
  p = fmaf(z, p, 4.1666666666666664e-02f);
  p = fmaf(z, p, -0.5f);
  const float c = fmaf(z, p, 1.0f);
  return flip ? -c : c;
}

// Heading of a food relative to the body axis, wrapped to [-pi, pi] (fp32): both angles are in [-pi, pi], so one multiple
// of 2 pi at most is off — round-to-nearest-even of rel / 2 pi is 0 on the closed interval, as snake:403-407's strict loops.
// Error on the circle for |th| <= pi: atan2_fast's plus the rounding of the difference and of the wrap, 2.2e-6 rad
// (PRECISE: 8.1e-7 rad, and 7.9e-7 on cos_wrapped of it, 4e-6 on a reward term of weight 5).  An injected heading up to
// SALP_SET_STATE_MAX_ANGLE = 100 rad that has not been wrapped by a step yet takes up to 16 turns out with an fp32 2 pi
// (1.7e-7 off per turn) from a difference rounded at ulp(64 .. 128) = 7.6e-6: 8e-6 rad = 2.5e-6 of pi, inside the contract.
template <bool PRECISE = false>
__device__ __forceinline__ float relative_heading(float dy, float dx, float th) {
  const float rel = atan2_fast<PRECISE>(dy, dx) - th;
  return fmaf(__builtin_rintf(rel * 0.15915494309189535f), -6.28318530717959f, rel);
}

}  // namespace salp
