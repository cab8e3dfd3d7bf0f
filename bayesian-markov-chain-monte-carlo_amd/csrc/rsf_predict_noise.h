// rsf_predict_noise.h — the posterior predictive band that includes the noise (include/rsf_predict_noise.h,
// rsf_predict_noise_quantiles): per output time k and probability p the root t of
//     F_k(t) = 1/n sum_i Phi((t - y_ki) / s_i) = p,        s_i = sqrt(std2_i),
// the kernels:
//   noise_params_kernel        per draw, once per call: s_i and r_i = 1 / (s_i sqrt 2), and the flag of a std2 that is not finite
//                              and > 0 (every writer stores the same value);
//   noise_quantile_row_kernel  one workgroup per output time.  Pass 0 reads the row once: the non-finite flag and, per target,
//                              min and max of y_i + z_p s_i, z_p = rank_ndtri(p): the exact bracket of the root.  Every later pass
//                              reads the row once for ALL targets that are still running and accumulates, per target, at its t
//                                  H = sum_i erfc(x_i),  D = sum_i exp(-x_i^2) r_i,   x_i = sg (y_i - t) r_i,
//                              sg = +1 for p <= 1/2 (H / 2n = F) and -1 for p > 1/2 (H / 2n = 1 - F, against q = 1 - p, exact): the
//                              sum is taken in the tail whose mass is the smaller, so its rounding is relative to min(p, 1 - p).
//                              One thread per target then updates its bracket from the sign of F - p and takes a Newton step on
//                              log(mass) = log q (step = mass log(mass / q) / F', F' = D / (n sqrt pi)) if it stays strictly
//                              inside the bracket and is at most half the previous step, a bisection otherwise (Numerical
//                              Recipes' rtsafe).
// A target stops when (a) |H / 2n - q| <= kNoiseTol q: the residual is at the rounding floor of the sum; (b) the Newton step is
// at most |t| 2^-52, one to two ulp: the step is taken (if it stays inside the bracket) and not evaluated; (c) no double lies
// strictly inside the bracket.  None of the three can alternate: the evaluated point becomes an end of the bracket on every pass,
// so no point is evaluated twice.
// A stopped target is skipped by a scalar branch and costs no erfc.  kNoiseMaxPasses caps the passes; a target still running
// then returns the midpoint of its bracket.
// Sums: per-thread strides over the row, then a butterfly over the wave's lanes, then the four waves in order; minima and maxima
// alike.  No float atomics, and a target's sums do not depend on which other targets share the pass: the same row, std2 and p
// give the same bits in any call.  fp64, no MFMA, no scratch: the targets' t live in SGPRs, their two sums in VGPRs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsf_kernel_common.h"
#include "rsf_rank_device.h"

namespace rsfk {

constexpr int kNoiseThreads = 256;
constexpr int kNoiseWaves = kNoiseThreads / 64;
constexpr int kNoiseMaxProbs = 16;    // RSF_PREDICT_MAX_PROBS
// RSF_PREDICT_NOISE_MAX_PASSES: pass 0, then at most 64 bisections and 64 Newton steps — a Newton step is taken only while the
// steps halve, and 64 halvings take a bracket or a step to 2^-64 of the first bracket, below the spacing of float64 at its ends
constexpr int kNoiseMaxPasses = 129;
// (a): 1.4e-14 of min(p, 1 - p); a fixed-order float64 sum of 2^18 terms is within 2e-15 of its value
constexpr double kNoiseTol = 0x1p-46;

struct NoiseArgs {
  int64_t n, nout;
  const double *series;   // [nout][n]
  const double *par;      // [2][n]: s, 1 / (s sqrt 2)
  const uint32_t *bad;    // != 0: a std2 is not finite and > 0
  double *out;            // [nprobs][nout]
  int32_t *passes;        // [nout]
  int32_t nprobs;
  double p[kNoiseMaxProbs];
};

__global__ void __launch_bounds__(256) noise_params_kernel(int64_t n, const double *__restrict__ std2, double *__restrict__ par,
                                                           uint32_t *__restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double s2 = std2[i];
  if (!(isfinite(s2) && s2 > 0.0)) *bad = 1u;
  const double s = sqrt(s2);
  par[i] = s;
  par[n + i] = 1.0 / (s * 1.41421356237309504880);
}

// a value that is the same in every lane, moved to scalar registers
__device__ __forceinline__ double noise_uniform(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  return __longlong_as_double((long long)((uint64_t)hi << 32 | lo));
}

// NP: the targets the unrolled loops provide for (4 or 16); the arithmetic of a target is the same in both
template <int NP>
__global__ void __launch_bounds__(kNoiseThreads) noise_quantile_row_kernel(NoiseArgs A) {
  __shared__ double red[2 * NP][kNoiseWaves];
  __shared__ double tt[NP], tlo[NP], thi[NP], tq[NP], tprev[NP], tres[NP];
  __shared__ uint32_t nonfinite, running, negative;  // bit j: target j still runs; its p > 1/2
  const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t n = A.n, k = blockIdx.x;
  const int np = A.nprobs;
  const double *row = A.series + k * n, *sd = A.par, *rs = A.par + n;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  // pass 0: the non-finite flag and every target's bracket
  if (t == 0) nonfinite = 0;
  double a[2 * NP];  // per target two accumulators: here -min and max, later H and D
  double z[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    z[j] = j < np ? noise_uniform(rank_ndtri(A.p[j])) : 0.0;
    a[2 * j] = a[2 * j + 1] = -__builtin_huge_val();
  }
  bool bad = false;
  for (int64_t i = t; i < n; i += kNoiseThreads) {
    const double y = row[i], s = sd[i];
    bad = bad || !isfinite(y);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      if (j < np) {
        const double e = y + z[j] * s;
        a[2 * j] = fmax(a[2 * j], -e);
        a[2 * j + 1] = fmax(a[2 * j + 1], e);
      }
    }
  }
  __syncthreads();
  if (bad) nonfinite = 1;  // (every writer stores the same value)
#pragma unroll
  for (int j = 0; j < 2 * NP; ++j) {
    if (j < 2 * np) {
      const double w = wave_all_ascending<true>(a[j]);
      if (lane == 0) red[j][wave] = w;
    }
  }
  __syncthreads();
  if (nonfinite || *A.bad) {
    if (t < (unsigned)np) A.out[(int64_t)t * A.nout + k] = nan;
    if (t == 0) A.passes[k] = 1;
    return;
  }
  if (t == 0) { running = np >= 32 ? ~0u : (1u << np) - 1u; negative = 0; }
  __syncthreads();
  if (t < (unsigned)np) {
    double lo = -fmax(fmax(red[2 * t][0], red[2 * t][1]), fmax(red[2 * t][2], red[2 * t][3]));
    double hi = fmax(fmax(red[2 * t + 1][0], red[2 * t + 1][1]), fmax(red[2 * t + 1][2], red[2 * t + 1][3]));
    // the ends are rounded sums and z_p is AS241's: a root within rounding of an end stays inside
    const double pad = 0x1p-49 * (fabs(lo) + fabs(hi));
    lo -= pad;
    hi += pad;
    const double p = A.p[t];
    if (p > 0.5) atomicOr(&negative, 1u << t);
    tq[t] = p > 0.5 ? 1.0 - p : p;
    tlo[t] = lo;
    thi[t] = hi;
    const double mid = lo + 0.5 * (hi - lo);
    tt[t] = tres[t] = mid;
    tprev[t] = hi - lo;
    if (!(mid > lo && mid < hi)) atomicAnd(&running, ~(1u << t));  // (c) already: n = 1 and p = 1/2, or every y + z s equal
  }
  __syncthreads();

  const double dn = (double)n;
  int passes = 1;
  for (; passes < kNoiseMaxPasses; ++passes) {
    const uint32_t run = __builtin_amdgcn_readfirstlane(running), neg = __builtin_amdgcn_readfirstlane(negative);
    if (!run) break;
    double tc[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      tc[j] = noise_uniform(tt[j < np ? j : 0]);
      a[2 * j] = a[2 * j + 1] = 0.0;
    }
    for (int64_t i = t; i < n; i += kNoiseThreads) {
      const double y = row[i], r = rs[i];
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        if (run >> j & 1u) {
          const double v = (y - tc[j]) * r;
          const double x = (neg >> j & 1u) ? -v : v;
          a[2 * j] += erfc(x);
          a[2 * j + 1] += exp(-(x * x)) * r;
        }
      }
    }
    __syncthreads();  // the previous pass' reads of red are over
#pragma unroll
    for (int j = 0; j < 2 * NP; ++j) {
      if (run >> (j >> 1) & 1u) {
        const double w = wave_all_ascending<false>(a[j]);
        if (lane == 0) red[j][wave] = w;
      }
    }
    __syncthreads();
    if (t < (unsigned)np && (run >> t & 1u)) {
      const double H = ((red[2 * t][0] + red[2 * t][1]) + red[2 * t][2]) + red[2 * t][3];
      const double D = ((red[2 * t + 1][0] + red[2 * t + 1][1]) + red[2 * t + 1][2]) + red[2 * t + 1][3];
      const double q = tq[t], x = tt[t];
      const double Hn = H / (2.0 * dn);
      const double g = Hn - q;                               // the mass of the smaller tail, minus its target
      const double fg = (neg >> t & 1u) ? -g : g;            // the sign of F - p
      const double fd = D * 0.56418958354775628695 / dn;     // F' = D / (n sqrt pi)
      double lo = tlo[t], hi = thi[t];
      if (fg < 0.0) lo = x;
      if (fg > 0.0) hi = x;
      tlo[t] = lo;
      thi[t] = hi;
      bool done = false;
      double res = x;
      if (fabs(g) <= kNoiseTol * q) {
        done = true;  // (a)
      } else {
        // Newton on log(mass) = log q: the tails of a normal mixture are close to exp(quadratic), on which the plain step crawls
        const double step = ((neg >> t & 1u) ? -Hn : Hn) * log1p(g / q) / fd;
        double xn = x - step;
        const bool inside = fd > 0.0 && xn > lo && xn < hi;
        if (fd > 0.0 && fabs(step) <= fabs(x) * 0x1p-52) {
          done = true;  // (b)
          if (inside) res = xn;
        } else if (!(inside && fabs(step) <= 0.5 * fabs(tprev[t]))) {
          xn = lo + 0.5 * (hi - lo);
          if (!(xn > lo && xn < hi)) done = true;  // (c)
        }
        if (!done) {
          tprev[t] = xn - x;
          tt[t] = xn;
          res = lo + 0.5 * (hi - lo);  // what the cap returns
        }
      }
      tres[t] = res;
      if (done) atomicAnd(&running, ~(1u << t));
    }
    __syncthreads();
  }
  if (t < (unsigned)np) A.out[(int64_t)t * A.nout + k] = tres[t];
  if (t == 0) A.passes[k] = passes;
}

}  // namespace rsfk
