// robot_math_host.cpp — host twin of the robot kernels' fp64 primitives (TEST INFRASTRUCTURE).
// Compiles csrc/salp_fp64_math.h as plain C++ (fma / rint from libm, -ffp-contract=off -fno-fast-math: oracle/Makefile)
// and runs its pure functions over arrays, in the layouts of salp_robot_math_probe.  A wavefront vote of the device is
// taken here over each group of 64 consecutive indices, which is the wavefront the probe puts them in.
#include "../underwater-swimmer_rl_amd/csrc/salp_fp64_math.h"

using namespace salp;

namespace {
constexpr int64_t kWave = 64;

template <class Pred>
bool group_any(int64_t g0, int64_t g1, Pred p) {
  bool any = false;
  for (int64_t i = g0; i < g1; ++i) any = any || p(i);
  return any;
}
}  // namespace

extern "C" {

double salp_math_host_rotate_max_step(void) { return kRotateMaxStep; }
double salp_math_host_euler_fold_above(void) { return kEulerFoldAbove; }

// Same arguments and layouts as salp_robot_math_probe, without the device id; -1 for a function that has no host form.
// `exact_steps` (nullable, CHAIN only): [steps][ceil(n / 64)] bytes, 1 where the group took the exact path at that step.
int salp_math_host(int function, const double* in, double* out, int64_t n, int32_t steps, uint8_t* exact_steps) {
  if (!in || !out || n < 1) return -1;
  const int64_t groups = (n + kWave - 1) / kWave;
  switch (function) {
    case SALP_MATH_SINCOS_SMALL:
      for (int64_t i = 0; i < n; ++i) sincos_small(in[i], out[i], out[n + i]);
      return 0;
    case SALP_MATH_SINCOS_EULER:
      for (int64_t g = 0; g < groups; ++g) {
        const int64_t g0 = g * kWave, g1 = g0 + kWave < n ? g0 + kWave : n;
        const bool fold = group_any(g0, g1, [&](int64_t i) { return fabs(in[i]) > kEulerFoldAbove; });
        for (int64_t i = g0; i < g1; ++i) sincos_euler(in[i], out[i], out[n + i], fold);
      }
      return 0;
    case SALP_MATH_ROTATE:
      for (int64_t i = 0; i < n; ++i) {
        double s = in[i], c = in[n + i];
        rotate_sincos(s, c, in[2 * n + i]);
        out[i] = s; out[n + i] = c;
      }
      return 0;
    case SALP_MATH_CHAIN: {
      if (steps < 0) return -1;
      double* s = out; double* c = out + n; double* e = out + 2 * n;
      for (int64_t g = 0; g < groups; ++g) {
        const int64_t g0 = g * kWave, g1 = g0 + kWave < n ? g0 + kWave : n;
        const bool fold0 = group_any(g0, g1, [&](int64_t i) { return fabs(in[i]) > kEulerFoldAbove; });
        for (int64_t i = g0; i < g1; ++i) { e[i] = in[i]; sincos_euler(e[i], s[i], c[i], fold0); }
        for (int32_t k = 0; k < steps; ++k) {
          const double* d = in + (int64_t)(1 + k) * n;
          for (int64_t i = g0; i < g1; ++i) e[i] += d[i];
          const bool exact = group_any(g0, g1, [&](int64_t i) { return fabs(d[i]) > kRotateMaxStep; });
          const bool fold = exact && group_any(g0, g1, [&](int64_t i) { return fabs(e[i]) > kEulerFoldAbove; });
          if (exact_steps) exact_steps[(int64_t)k * groups + g] = exact ? 1 : 0;
          for (int64_t i = g0; i < g1; ++i) {
            double s1 = 0.0, c1 = 1.0, s2 = 0.0, c2 = 1.0;   // the other two angles stay zero
            advance_euler_sincos(e[i], 0.0, 0.0, d[i], 0.0, 0.0, s[i], c[i], s1, c1, s2, c2, exact, fold, false, false);
          }
        }
      }
      return 0;
    }
    default:
      return -1;
  }
}

}  // extern "C"
