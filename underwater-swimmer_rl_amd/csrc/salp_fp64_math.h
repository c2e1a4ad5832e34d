// salp_fp64_math.h — the hand-written fp64 math of the robot kernels (salp_robot_kernels.h, salp_robot_cycle_body.h):
// sin / cos with its own argument reduction, the carried sin / cos of the Euler angles, and Newton-refined
// reciprocal / square root.  They replace the device library's routines on a path bound by the fp64 VALU rate, and
// each has a stated error bound that tests/test_robot_math.py (against mpmath) and tests/test_gpu_robot_math.py
// (device against the host twin bit for bit, rcp / sqrt against exact references) enforce.
//
// The header compiles in two ways:
//   * as device code (hipcc): what the kernels include, through salp_device.h or directly;
//   * as plain host C++ (tests/robot_math_host.cpp, the "host twin"): the pure functions with fma / rint from <cmath>.
//     A wavefront vote (__any on the device) is an explicit bool parameter there, taken by the caller over the 64
//     indices it treats as one wavefront.  rcp_nr / sqrt_nr are device-only: their seeds are hardware instructions.
// Every multiply-add that is fused is written as fma(); the units are compiled with -ffp-contract=off, so device and
// host twin round in the same places and agree bit for bit.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SALP_MATH_DEVICE 1
#define SALP_MATH_FN __device__ __forceinline__
// a wavefront vote: __any of the predicate; no parameter
#define SALP_VOTE_PARAM(name)
#define SALP_VOTE_PASS(name)
#define SALP_VOTE(pred, name) __any(pred)
#else
#include <cmath>
#define SALP_MATH_FN inline
// the host twin: the caller's vote, one more bool parameter
#define SALP_VOTE_PARAM(name) , bool name
#define SALP_VOTE_PASS(name) , name
#define SALP_VOTE(pred, name) (name)
#endif
#include <stdint.h>

namespace salp {

#ifndef SALP_MATH_DEVICE
using std::fabs;
using std::fma;
#endif

// sin and cos of x: Cody-Waite reduction by pi/2 with fused multiply-adds against a 33 + 53 bit split of pi/2 (the
// quadrant count fn stays below 2^31 and fn * PIO2_1 is exact up to |x| ~ 1e9) and the fdlibm kernel polynomials on
// [-pi/4, pi/4].  Absolute error <= 2^-52 (one ulp of 1) for |x| <= 1e9; measured 1.1e-16.  Not a bound in ulps of
// the result: 1.35 ulp at x ~ 1.048, and arbitrarily many next to a zero of sin or cos.  Explicit fma() is allowed
// here because these values have no bit-exact counterpart on the CPU anyway (glibc's sin/cos are a different
// algorithm).
SALP_MATH_FN void sincos_small(double x, double& s, double& c) {
  const double fn = __builtin_rint(x * 6.36619772367581382433e-01);
  double r = fma(-fn, 1.57079632673412561417e+00, x);
  r = fma(-fn, 6.07710050650619224932e-11, r);
  const double z = r * r;
  // kernel sin
  double ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  ps = fma(z, ps, 2.75573137070700676789e-06);
  ps = fma(z, ps, -1.98412698298579493134e-04);
  ps = fma(z, ps, 8.33333333332248946124e-03);
  const double v = z * r;
  const double sr = fma(v, fma(z, ps, -1.66666666666666324348e-01), r);
  // kernel cos
  double pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  pc = fma(z, pc, -2.75573143513906633035e-07);
  pc = fma(z, pc, 2.48015872894767294178e-05);
  pc = fma(z, pc, -1.38888888888741095749e-03);
  pc = fma(z, pc, 4.16666666666666019037e-02);
  const double hz = 0.5 * z;
  const double w = 1.0 - hz;
  const double cr = w + (((1.0 - w) - hz) + z * (z * pc));
  const int q = (int)fn & 3;
  const double s0 = (q & 1) ? cr : sr;
  const double c0 = (q & 1) ? sr : cr;
  s = (q & 2) ? -s0 : s0;
  c = ((q + 1) & 2) ? -c0 : c0;
}

// sin/cos of an Euler angle.  The angles are unbounded (yaw winds up).  sincos_small is good to |x| ~ 1e9; past
// kEulerFoldAbove = 1e8 rad anywhere in the wavefront (wave-uniform test) the angle is first folded into [-pi, pi]
// against a double-double 2*pi.  The folded angle is rounded to a double of magnitude up to pi, which alone costs up
// to 2^-52 rad; with sincos_small's 2^-52 the total absolute error is <= 2^-51 up to |x| ~ 1e15 (measured 2.8e-16).
constexpr double kEulerFoldAbove = 1.0e8;
SALP_MATH_FN void sincos_euler(double x, double& s, double& c SALP_VOTE_PARAM(fold_any)) {
  if (SALP_VOTE(fabs(x) > kEulerFoldAbove, fold_any)) {
    const double k = __builtin_rint(x * 0.15915494309189535);
    x = fma(-k, 2.4492935982947064e-16, fma(-k, 6.283185307179586, x));
  }
  sincos_small(x, s, c);
}

// (s, c) <- sin / cos of (angle + d) from sin / cos of the angle, |d| <= kRotateMaxStep: Taylor polynomials of sin d
// (to d^9) and cos d (to d^10) and the angle-addition formulas; ~16 operations instead of a full sincos.  The first
// dropped terms are d^11 / 11! and d^12 / 12!: 2.9e-18 at |d| = 0.125 (6.0e-15 at 0.25, below 1e-16 only for
// |d| < 0.172).  One call from a correctly rounded (s, c) is within 4 * 2^-53 plus that term of the exact values.
// Carried over the 1460 steps of the longest cycle the pair stays within 1e-12 of sin / cos of the exact angle with
// this threshold (measured 6.7e-14 at a constant 0.125; a threshold of 0.25 gave 8.7e-12).
constexpr double kRotateMaxStep = 0.125;
SALP_MATH_FN void rotate_sincos(double& s, double& c, double d) {
  const double z = d * d;
  double ps = fma(z, 2.7557319223985893e-06, -1.9841269841269841e-04);    // 1/9!, -1/7!
  ps = fma(z, ps, 8.3333333333333332e-03);
  ps = fma(z, ps, -1.6666666666666666e-01);
  const double sd = fma(d * z, ps, d);
  double pc = fma(z, -2.7557319223985888e-07, 2.4801587301587302e-05);    // -1/10!, 1/8!
  pc = fma(z, pc, -1.3888888888888889e-03);
  pc = fma(z, pc, 4.1666666666666664e-02);
  pc = fma(z, pc, -0.5);
  const double cd = fma(z, pc, 1.0);
  const double ns = fma(s, cd, c * sd), nc = fma(c, cd, -(s * sd));
  s = ns; c = nc;
}

// One Euler step of the carried sin / cos pairs of the three Euler angles: (sp, cp), (st, ct), (ss, cs) belong to the
// angles before the step, e0..e2 are the angles after it and d0..d2 the increments just added.  An increment above
// kRotateMaxStep anywhere in the wavefront takes the exact path for that step, for all three angles of every lane.
SALP_MATH_FN void advance_euler_sincos(double e0, double e1, double e2, double d0, double d1, double d2,
                                       double& sp, double& cp, double& st, double& ct, double& ss, double& cs
                                       SALP_VOTE_PARAM(exact_any) SALP_VOTE_PARAM(fold0_any) SALP_VOTE_PARAM(fold1_any)
                                       SALP_VOTE_PARAM(fold2_any)) {
  if (SALP_VOTE(fabs(d0) > kRotateMaxStep || fabs(d1) > kRotateMaxStep || fabs(d2) > kRotateMaxStep, exact_any)) {
    sincos_euler(e0, sp, cp SALP_VOTE_PASS(fold0_any));
    sincos_euler(e1, st, ct SALP_VOTE_PASS(fold1_any));
    sincos_euler(e2, ss, cs SALP_VOTE_PASS(fold2_any));
  } else {
    rotate_sincos(sp, cp, d0);
    rotate_sincos(st, ct, d1);
    rotate_sincos(ss, cs, d2);
  }
}

#ifdef SALP_MATH_DEVICE
// 1/x for a normal, finite x whose reciprocal is normal too: v_rcp_f64 and two Newton steps (<= 1 ulp of the exact
// value; no range scaling / fix-up pass)
SALP_MATH_FN double rcp_nr(double x) {
  double y = __builtin_amdgcn_rcp(x);
  double e = fma(-x, y, 1.0);
  y = fma(y, e, y);
  e = fma(-x, y, 1.0);
  return fma(y, e, y);
}
// sqrt(x) for x = 0 or x well inside the normal range: v_rsq_f64, two coupled Newton steps and a final
// residual correction (<= 1 ulp); tiny arguments anywhere in the wavefront take the library routine (wave-uniform
// test), which rounds correctly
SALP_MATH_FN double sqrt_nr(double x) {
  if (__any(x < 1.0e-200 && x != 0.0)) return sqrt(x);
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double rr = fma(-h, g, 0.5);
  g = fma(g, rr, g); h = fma(h, rr, h);
  const double rr2 = fma(-h, g, 0.5);
  g = fma(g, rr2, g); h = fma(h, rr2, h);
  const double d = fma(-g, g, x);
  g = fma(d, h, g);
  return x == 0.0 ? 0.0 : g;
}
#endif

}  // namespace salp

// ---- test support ---------------------------------------------------------------------------------------------------
// salp_robot_math_probe (salp_robot.hip; its kernel is in salp_robot_kernels.h) runs one of the functions above on the device, element i on thread i of
// 256-thread blocks, so wavefront w holds the elements [64 w, 64 w + 64) and a test can put a lane that triggers a
// wave-uniform fallback into a wavefront of its choice.  tests/robot_math_host.cpp is the same call on the host, a
// group of 64 indices voting like a wavefront.  Not part of the public ABI (include/salp_robot.h).
//   function              in                                out
//   SINCOS_SMALL / EULER  x [n]                             s, c [2][n]
//   ROTATE                s, c, d [3][n]                    s, c [2][n]
//   CHAIN                 x0 [n], then d [steps][n]         s, c, angle [3][n]: sincos_euler(x0), then per step
//                                                           angle += d and advance_euler_sincos (the angle as roll, the
//                                                           other two angles zero)
//   RCP_NR / SQRT_NR      x [n]                             y [n]  (device only)
enum {
  SALP_MATH_SINCOS_SMALL = 0, SALP_MATH_SINCOS_EULER = 1, SALP_MATH_ROTATE = 2, SALP_MATH_CHAIN = 3,
  SALP_MATH_RCP_NR = 4, SALP_MATH_SQRT_NR = 5
};
// `in` / `out` are host arrays; `steps` is read by CHAIN only.  0 on success, negative with salp_robot_last_error() set.
extern "C" int salp_robot_math_probe(int device_id, int function, const double* in, double* out, int64_t n, int32_t steps);
