// rsf_kernels_pool.h — posterior post-processing of the pooled draws: pool_moments_kernel, pool_hist_kernel,
// pool_hist_finish_kernel, pool_kde_kernel; and the last step of every unit's reductions, sum_in_order_kernel and
// sum_strided_tree_kernel, which the other units reach through rsfh::sum_in_order / sum_strided_tree (rsf_host.h).
// Included by rsf_pool.hip only (none of these kernels is a template).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsf_kernel_common.h"
#include "rsf_math.h"

namespace rsfk {

// ---------------------------------------------------------------------------------------------
// posterior post-processing on pooled samples (RSF.plot_dist, RSF.py:717-746)
// ---------------------------------------------------------------------------------------------
constexpr int kPoolBlocks = 1024;  // 4 workgroups per CU; partials are combined deterministically (no atomics)

struct PoolPartial {
  double cnt, sum, sumsq, mn, mx;  // sums are taken about a common shift for stability
};

__global__ void __launch_bounds__(kMaxBlock)
pool_moments_kernel(int64_t n, const double *__restrict__ x, int64_t stride, double shift, PoolPartial *__restrict__ part) {
  __shared__ PoolPartial sh[kMaxBlock / 64];
  double cnt = 0.0, sum = 0.0, sumsq = 0.0, mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = x[i * stride], dlt = v - shift;
    cnt += 1.0; sum += dlt; sumsq = __builtin_fma(dlt, dlt, sumsq);
    mn = fmin(mn, v); mx = fmax(mx, v);
  }
  cnt = wave_sum(cnt); sum = wave_sum(sum); sumsq = wave_sum(sumsq);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { mn = fmin(mn, __shfl_down(mn, off, 64)); mx = fmax(mx, __shfl_down(mx, off, 64)); }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = {cnt, sum, sumsq, mn, mx};
  __syncthreads();
  if (threadIdx.x == 0) {
    PoolPartial p = sh[0];
    for (unsigned w = 1; w < blockDim.x / 64; ++w) {
      p.cnt += sh[w].cnt; p.sum += sh[w].sum; p.sumsq += sh[w].sumsq; p.mn = fmin(p.mn, sh[w].mn); p.mx = fmax(p.mx, sh[w].mx);
    }
    part[blockIdx.x] = p;
  }
}

// Fixed-bin histogram (rsf_pool_histogram): HBM-bound, one pass.  Every workgroup counts into an LDS copy of the bins
// (ds_add_u32), then adds its non-empty bins to the global 64-bit counters — integer atomics, so the result does not
// depend on the order of arrival.  The bin of a sample is numpy.histogram's, edge cases included: a first guess
// floor((x - lo) * nbins/(hi - lo)), then numpy's own correction against the bin EDGES np.linspace(lo, hi, nbins + 1)
// (edge b = b * step + lo, two roundings — formed here with contraction switched off), so that a sample
// sitting exactly on an edge — a chain that rejects repeats values like q0 — lands where numpy puts it.
constexpr int kHistMaxBins = 4096;

__device__ __forceinline__ double hist_edge(int b, double lo, double hi, double step, int nbins) {
#pragma clang fp contract(off)  // numpy's edge is a product rounded, then a sum rounded: no fused multiply-add here
  const double m = (double)b * step;
  return b == nbins ? hi : m + lo;
}

__device__ __forceinline__ int hist_bin(double v, double lo, double hi, double scale, double step, int nbins) {
  if (v < lo) return 0;
  if (!(v <= hi)) return nbins + 1;                      // above hi, or NaN
  int b = (int)((v - lo) * scale);
  b = b < nbins ? b : nbins - 1;                         // v == hi (or rounding at the upper edge) -> last bin
  if (v < hist_edge(b, lo, hi, step, nbins)) --b;        // the guess is within one bin of the truth; the edges decide
  if (b != nbins - 1 && v >= hist_edge(b + 1, lo, hi, step, nbins)) ++b;
  return 1 + b;
}

__global__ void __launch_bounds__(kMaxBlock)
pool_hist_kernel(int64_t n, const double *__restrict__ x, int64_t stride, int nbins, double lo, double hi, double scale, double step,
                 unsigned long long *__restrict__ counts) {
  extern __shared__ unsigned int hbins[];
  for (int b = threadIdx.x; b < nbins + 2; b += blockDim.x) hbins[b] = 0u;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&hbins[hist_bin(x[i * stride], lo, hi, scale, step, nbins)], 1u);
  __syncthreads();
  for (int b = threadIdx.x; b < nbins + 2; b += blockDim.x)
    if (hbins[b]) atomicAdd(&counts[b], (unsigned long long)hbins[b]);
}

__global__ void __launch_bounds__(kMaxBlock) pool_hist_finish_kernel(int nb, const unsigned long long *__restrict__ counts, double *__restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < nb) out[b] = (double)counts[b];
}

// Each workgroup owns a contiguous slice of the samples, streamed through LDS in tiles; every thread
// accumulates the kernel sum of its grid points over the slice (LDS broadcast reads).  partial[block][m].
constexpr int kKdeTile = 1024;

__global__ void __launch_bounds__(kMaxBlock)
pool_kde_kernel(int64_t n, const double *__restrict__ x, int64_t stride, int m, const double *__restrict__ grid, double inv2c,
                double *__restrict__ partial) {
  __shared__ double tile[kKdeTile];
  const int64_t per = (n + gridDim.x - 1) / gridDim.x, lo = (int64_t)blockIdx.x * per, hi = min(n, lo + per);
  for (int j0 = 0; j0 < m; j0 += blockDim.x) {
    const int j = j0 + threadIdx.x;
    const double g = j < m ? grid[j] : 0.0;
    double acc = 0.0;
    for (int64_t t0 = lo; t0 < hi; t0 += kKdeTile) {
      const int tn = (int)min((int64_t)kKdeTile, hi - t0);
      __syncthreads();
      for (int t = threadIdx.x; t < tn; t += blockDim.x) tile[t] = x[(t0 + t) * stride];
      __syncthreads();
      for (int t = 0; t < tn; ++t) {
        const double dlt = g - tile[t];
        acc += rsf::fm::exp(-dlt * dlt * inv2c);
      }
    }
    if (j < m) partial[(int64_t)blockIdx.x * m + j] = acc;
  }
}

// ---- the last step of a reduction: the workgroups' partials part[b][nf], summed in one of two fixed orders --------------
// In index order, one thread per field f = blockIdx.x * 256 + threadIdx.x, slab s = blockIdx.y of `per` partials:
// out[s][f] = scale * (0.0 + part[s per][f] + part[s per + 1][f] + ...) up to the slab's or the partials' end.  A scale of 1.0
// changes no bit.
__global__ void __launch_bounds__(kMaxBlock)
sum_in_order_kernel(int64_t nblocks, int64_t per, int64_t nf, const double *__restrict__ part, double scale, double *__restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int64_t b0 = (int64_t)blockIdx.y * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
  double t = 0.0;
  for (int64_t b = b0; b < b1; ++b) t += part[b * nf + f];
  out[(int64_t)blockIdx.y * nf + f] = t * scale;
}

// Strided, then a tree, one workgroup per field f = blockIdx.x: thread t takes the partials t, t + 256, ... in that order from
// 0.0, then wave_sum and the waves in index order.  (One thread per field walking all 1024 partials of a few fields took longer
// than the pass over the pool that made them.)
__global__ void __launch_bounds__(kMaxBlock) sum_strided_tree_kernel(int nblocks, int nf, const double *__restrict__ part, double *__restrict__ out) {
  __shared__ double sh[kMaxBlock / 64];
  const int f = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) s += part[(int64_t)b * nf + f];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (unsigned w = 1; w < blockDim.x / 64; ++w) s += sh[w];
    out[f] = s;
  }
}

}  // namespace rsfk
