// rsf_psis.h — PSIS-LOO and the Pareto shape of pooled draws (include/rsf_psis.h, rsf_predict_psis_loo), the kernels:
//   psis_params_kernel  per draw, once per call: 1/2 log(2 pi s2) and 1/(2 s2), so that x_ik = -l_ik is two reads and three
//                       operations wherever a row is read (the log-likelihood matrix is never stored);
//   psis_row_kernel     one workgroup per output time, every step of the definition (tests/psis_reference.py):
//     1. one read of the row: max_i x_i and the non-finite flag;
//     2. eight reads: the order statistic x_(n - tail_len - 1) of x - max by rank_select (rsf_diag_rank.h) with one target rank;
//     3. one read: the members above the cutoff go to LDS (integer atomic for the slot: the tail is sorted next, so the order
//        of arrival changes nothing), the body's sum exp(x) and sum exp(2 x) are accumulated;
//     4. LDS bitonic sort of the tail (of the raw x, from which l = -x is exact), then t_j = exp(x_j) - exp(cutoff);
//     5. Zhang and Stephens' fit: the m candidates go round the workgroup's waves, each a strided sum over the tail and a
//        wave butterfly; the weights, one thread per candidate; b, then k with the whole workgroup;
//     6. the smoothed values and the final sums.
// For a member that is not smoothed lw_i + l_i = -max - logsumexp(x) for every i, so
//     elpd_loo_k = -max - logsumexp(x) + log(n - n_tail + sum_tail exp(x_new_j - x_j)),
// which needs no exponential per body member.  fp64, no MFMA, no scratch.  Every floating-point sum has a fixed order — per-thread
// strides, then a fixed tree — and there is no float atomic: the same input gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsf_kernel_common.h"
#include "rsf_rank_device.h"

namespace rsfk {

constexpr int kPsisThreads = 256;
constexpr int kPsisWaves = kPsisThreads / 64;
constexpr int kPsisMaxTail = 8192;     // RSF_PSIS_MAX_TAIL: two arrays of that many doubles are 128 KiB of the CU's 160 KiB of LDS
constexpr int kPsisMaxCand = 30 + 90;  // m = 30 + floor(sqrt(N)), N <= kPsisMaxTail
constexpr int kPsisOut = 4;            // RSF_PSIS_OUT
constexpr double kPsisLogDblMin = -708.39641853226410622;  // log(DBL_MIN)

__global__ void __launch_bounds__(256) psis_params_kernel(int64_t n, const double *__restrict__ std2, double *__restrict__ par) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double s2 = std2[i];
  par[i] = 0.5 * log(6.283185307179586476925 * s2);
  par[n + i] = 0.5 / s2;
}

// fixed tree over the workgroup's per-thread values; the result in every thread.  red: kPsisThreads doubles of LDS
template <bool MAX>
__device__ __forceinline__ double psis_block_reduce(double v, double *red) {
  const unsigned t = threadIdx.x;
  __syncthreads();  // the previous use of red is over
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = kPsisThreads / 2; s > 0; s >>= 1) {
    if (t < (unsigned)s) red[t] = MAX ? fmax(red[t], red[t + s]) : red[t] + red[t + s];
    __syncthreads();
  }
  return red[0];
}

struct PsisArgs {
  int64_t n, nout;
  const double *series;  // [nout][n]
  const double *par;     // [2][n]: 1/2 log(2 pi s2), 1/(2 s2)
  const double *data;    // [nout]
  double *out;           // [nout][kPsisOut]
  int32_t tail_len;      // ceil(min(0.2 n, 3 sqrt(n / r_eff))), <= kPsisMaxTail
  int32_t cap;           // the power of two >= tail_len: each of the two LDS arrays
};

__global__ void __launch_bounds__(kPsisThreads) psis_row_kernel(PsisArgs A) {
  extern __shared__ __attribute__((aligned(16))) double psis_lds[];
  __shared__ double red[kPsisThreads];
  __shared__ double cb[kPsisMaxCand], cL[kPsisMaxCand], cw[kPsisMaxCand];
  __shared__ RankSelect<1> sel;
  __shared__ uint32_t nonfinite, ntail;
  __shared__ double fit[2];  // b, then pareto_k and sigma
  double *xs = psis_lds, *ts = psis_lds + A.cap;  // the tail's raw x, ascending; t_j
  const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t n = A.n, k = blockIdx.x;
  const double *row = A.series + k * n, *ln = A.par, *hh = A.par + n;
  const double obs = A.data[k];
  double *out = A.out + k * kPsisOut;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  auto xraw = [&](int64_t i) {
    const double r = obs - row[i];
    return ln[i] + (r * r) * hh[i];
  };

  // 1. the maximum, and whether every x is finite
  if (t == 0) { nonfinite = 0; ntail = 0; }
  double mx = -__builtin_huge_val();
  bool bad = false;
  for (int64_t i = t; i < n; i += kPsisThreads) {
    const double x = xraw(i);
    bad = bad || !isfinite(x);
    mx = fmax(mx, x);
  }
  __syncthreads();
  if (bad) nonfinite = 1;  // (every writer stores the same value)
  mx = psis_block_reduce<true>(mx, red);
  if (nonfinite) {
    if (t < kPsisOut) out[t] = nan;
    return;
  }

  // 2. x_(j0) of x - max by radix select
  if (t == 0) {
    const int64_t j0 = n - A.tail_len - 1;
    sel.want[0] = (uint32_t)(j0 < 0 ? 0 : j0);
  }
  rank_select(sel, 1, n, [&](int64_t i, int) { return rank_key(xraw(i) - mx); });
  const double cutoff = fmax(rank_value(sel.prefix[0]), kPsisLogDblMin);

  // 3. the tail to LDS; the body's sums
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = t; i < n; i += kPsisThreads) {
    const double xr = xraw(i), x = xr - mx;
    if (x > cutoff) {
      const uint32_t slot = atomicAdd(&ntail, 1u);
      if (slot < (uint32_t)A.cap) xs[slot] = xr;  // (at most tail_len members lie strictly above x_(n - tail_len - 1))
    } else {
      const double e = exp(x);
      s1 += e;
      s2 += e * e;
    }
  }
  s1 = psis_block_reduce<false>(s1, red);
  s2 = psis_block_reduce<false>(s2, red);
  const int N = (int)(ntail < (uint32_t)A.cap ? ntail : (uint32_t)A.cap);
  double pareto_k = __builtin_huge_val();
  double q = (double)N;  // sum over the tail of exp(x_new - x): N while nothing is smoothed
  double e1 = 0.0, e2 = 0.0;  // the tail's sum exp(x_new), sum exp(2 x_new)
  bool smoothed = false;

  if (N > 4) {
    // 4. sort, then t_j
    int P = 8;
    while (P < N) P <<= 1;
    for (int i = N + (int)t; i < P; i += kPsisThreads) xs[i] = __builtin_huge_val();
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int i = t; i < P; i += kPsisThreads) {
          const int o = i ^ j;
          if (o > i) {
            const double a = xs[i], b = xs[o];
            if (((i & kk) == 0) == (a > b)) { xs[i] = b; xs[o] = a; }
          }
        }
        __syncthreads();
      }
    }
    const double ecut = exp(cutoff);
    for (int i = t; i < N; i += kPsisThreads) ts[i] = exp(xs[i] - mx) - ecut;
    __syncthreads();

    // 5. the fit
    const int m = 30 + (int)floor(sqrt((double)N));
    const double dN = (double)N;
    const double tq = ts[(int)(dN / 4.0 + 0.5) - 1], tmax = ts[N - 1];
    for (int j = wave; j < m; j += kPsisWaves) {
      double b = 1.0 - sqrt((double)m / ((double)(j + 1) - 0.5));
      b /= 3.0 * tq;
      b += 1.0 / tmax;
      double s = 0.0;
      for (int i = lane; i < N; i += 64) s += log1p(-b * ts[i]);
      const double kj = wave_all_ascending<false>(s) / dN;
      if (lane == 0) {
        cb[j] = b;
        cL[j] = dN * (log(-b / kj) - kj - 1.0);
      }
    }
    __syncthreads();
    if (t < (unsigned)m) {
      const double Lj = cL[t];
      double s = 0.0;
      for (int l = 0; l < m; ++l) s += exp(cL[l] - Lj);
      cw[t] = 1.0 / s;
    }
    __syncthreads();
    if (t == 0) {
      double sw = 0.0, b = 0.0;
      for (int j = 0; j < m; ++j) sw += cw[j] >= 10.0 * 2.220446049250313e-16 ? cw[j] : 0.0;
      for (int j = 0; j < m; ++j) b += cw[j] >= 10.0 * 2.220446049250313e-16 ? (cw[j] / sw) * cb[j] : 0.0;
      fit[0] = b;
    }
    __syncthreads();
    const double b = fit[0];
    double s = 0.0;
    for (int i = t; i < N; i += kPsisThreads) s += log1p(-b * ts[i]);
    const double kbar = psis_block_reduce<false>(s, red) / dN;
    const double sigma = -kbar / b;
    pareto_k = (dN * kbar + 5.0) / (dN + 10.0);

    // 6. the smoothed tail
    if (isfinite(pareto_k)) {
      smoothed = true;
      double sq = 0.0;
      for (int j = t; j < N; j += kPsisThreads) {
        const double p = ((double)j + 0.5) / dN;
        const double xn = fmin(log(sigma * expm1(-pareto_k * log1p(-p)) / pareto_k + ecut), 0.0);
        const double e = exp(xn);
        e1 += e;
        e2 += e * e;
        sq += exp(xn - (xs[j] - mx));
      }
      e1 = psis_block_reduce<false>(e1, red);
      e2 = psis_block_reduce<false>(e2, red);
      q = psis_block_reduce<false>(sq, red);
    }
  }
  if (!smoothed) {  // the tail keeps its x (all <= 0 after the maximum was subtracted)
    for (int j = t; j < N; j += kPsisThreads) {
      const double e = exp(xs[j] - mx);
      e1 += e;
      e2 += e * e;
    }
    e1 = psis_block_reduce<false>(e1, red);
    e2 = psis_block_reduce<false>(e2, red);
  }
  if (t == 0) {
    const double w1 = s1 + e1, w2 = s2 + e2;
    out[0] = (-mx - log(w1)) + log((double)(n - N) + q);
    out[1] = pareto_k;
    out[2] = (double)N;
    out[3] = (w1 * w1) / w2;
  }
}

}  // namespace rsfk
