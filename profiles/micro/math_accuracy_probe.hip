// Accuracy of the device library's fp32 functions that the sampling policy arithmetic calls (csrc/salp_policy.h:
// logf, sqrtf, cospif for the noise; expf, log1pf, tanhf for the sample and its log-probability), each ALONE against
// float64 on the host, on the arguments that arithmetic can reach.  No kernel of the library is involved.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -o math_accuracy_probe math_accuracy_probe.hip
//   ./math_accuracy_probe        -> one JSON line
// Unit: |computed - exact| / (2^-23 |exact|) (at least the error in ulps of the exact value: an ulp is at most 2^-23 |value|);
// `zero_miss`: arguments whose exact value is 0 and whose computed value is not.  policy.py's ULP_* constants are twice the
// figures printed here (profiles/r07/ab_notes.md).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

enum { F_LOG = 0, F_SQRT, F_COSPI, F_EXP, F_LOG1P, F_TANH };

__global__ void eval_kernel(int fn, const float* __restrict__ in, float* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float x = in[i];
    float y;
    switch (fn) {
      case F_LOG: y = logf(x); break;
      case F_SQRT: y = sqrtf(x); break;
      case F_COSPI: y = cospif(x); break;
      case F_EXP: y = expf(x); break;
      case F_LOG1P: y = log1pf(x); break;
      default: y = tanhf(x); break;
    }
    out[i] = y;
  }
}

#define CHECK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_)); return 1; } } while (0)

// cos(pi x) for x = k 2^-23, k in [0, 2^24): the argument reduced exactly by quarter turns
static double cospi_exact(float x) {
  const long k = (long)((double)x * 8388608.0);            // exact: x is a multiple of 2^-23
  const long q = k >> 22;
  const double r = (double)(k & ((1L << 22) - 1)) / 8388608.0;
  const double c = cos(M_PI * r), s = sin(M_PI * r);
  return q == 0 ? c : (q == 1 ? -s : (q == 2 ? -c : s));
}

static double exact_of(int fn, float x) {
  switch (fn) {
    case F_LOG: return log((double)x);
    case F_SQRT: return sqrt((double)x);
    case F_COSPI: return cospi_exact(x);
    case F_EXP: return exp((double)x);
    case F_LOG1P: return log1p((double)x);
    default: return tanh((double)x);
  }
}

int main() {
  const size_t N = (size_t)1 << 24;
  std::vector<float> in(N + 127 * 4096), out(in.size());
  float *d_in = nullptr, *d_out = nullptr;
  CHECK(hipMalloc((void**)&d_in, in.size() * sizeof(float)));
  CHECK(hipMalloc((void**)&d_out, in.size() * sizeof(float)));
  const char* names[] = {"logf", "sqrtf", "cospif", "expf", "log1pf", "tanhf"};
  std::vector<float> logs(N);      // logf of every u1, as computed on the device: sqrtf's arguments are -2 times these
  printf("{");
  for (int fn = 0; fn <= F_TANH; ++fn) {
    size_t n = N;
    for (size_t k = 0; k < N; ++k) {
      switch (fn) {
        case F_LOG: in[k] = (float)(k + 1) * 5.9604644775390625e-8f; break;                  // every u1 = (k + 1) 2^-24
        case F_SQRT: in[k] = -2.0f * logs[k]; break;                                          // every reachable -2 logf(u1)
        case F_COSPI: in[k] = 2.0f * ((float)k * 5.9604644775390625e-8f); break;              // every 2 u2
        case F_EXP: in[k] = -80.0f + 82.0f * (float)((double)k / (double)(N - 1)); break;     // [-80, 2]: both uses (ls; -|2u|)
        case F_LOG1P: in[k] = (float)k * 5.9604644775390625e-8f; break;                       // [0, 1)
        default: in[k] = -20.0f + 40.0f * (float)((double)k / (double)(N - 1)); break;        // [-20, 20]
      }
    }
    if (fn == F_LOG1P)     // and small arguments (exp(-|2u|) for large |u|): 2^-e (1 + m 2^-12), e = 0 .. 126
      for (int e = 0; e <= 126; ++e)
        for (int m = 0; m < 4096; ++m) in[n++] = ldexpf(1.0f + (float)m / 4096.0f, -e);
    CHECK(hipMemcpy(d_in, in.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(eval_kernel, dim3(1024), dim3(256), 0, 0, fn, (const float*)d_in, d_out, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, n * sizeof(float), hipMemcpyDeviceToHost));
    if (fn == F_LOG) for (size_t k = 0; k < N; ++k) logs[k] = out[k];
    double worst = 0.0;
    float worst_x = 0.f;
    size_t zero_miss = 0, bad = 0;
    for (size_t k = 0; k < n; ++k) {
      const double ex = exact_of(fn, in[k]);
      const double got = (double)out[k];
      if (!(got == got)) { ++bad; continue; }
      if (ex == 0.0) { zero_miss += (got != 0.0); continue; }
      const double r = fabs(got - ex) / (ldexp(1.0, -23) * fabs(ex));
      if (r > worst) { worst = r; worst_x = in[k]; }
    }
    printf("%s\"%s\": {\"max_err\": %.4f, \"at\": %.9g, \"zero_miss\": %zu, \"nan\": %zu, \"points\": %zu}", fn ? ", " : "",
           names[fn], worst, (double)worst_x, zero_miss, bad, n);
  }
  printf("}\n");
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return 0;
}
