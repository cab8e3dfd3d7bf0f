// rsf_kernels_joint.h — the joint posterior of the pooled draws (include/rsf_joint.h): pool_joint_moments_kernel,
// pool_hist2d_kernel, pool_kde2d_kernel.  Included by rsf_pool.hip only, after rsf_kernels_pool.h, whose hist_bin,
// pool_hist_finish_kernel, sum_strided_tree_kernel (the moments' last step) and sum_in_order_kernel (the KDE's) these share.
//
// Reproducibility: every sum below has an order fixed by the shape of the input and the launch geometry (grid and block sizes,
// which the host derives from n, d and m alone) — per thread in row order, per wave by the shuffle tree, the waves of a
// workgroup and the workgroups' partials in index order — and the only atomics are integer ones.  Nothing depends on the order of arrival.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_joint.h"
#include "rsf_kernel_common.h"
#include "rsf_kernels_pool.h"
#include "rsf_math.h"

namespace rsfk {

constexpr int joint_fields(int d) { return RSF_JOINT_PARTIALS(d); }

// where the columns lie and what they are centred on: a kernel argument, so that c[p] and col[p] are scalar registers
struct JointCols {
  double c[RSF_JOINT_MAX_PARAMS];
  int32_t col[RSF_JOINT_MAX_PARAMS];
  int64_t ld;  // doubles from one row to the next
};

// One pass, HBM-bound: every thread holds the running sums of its rows about the centre — d first and d (d + 1) / 2 second
// moments, a count and the count of left-out rows — in registers.  D = 1, 2, 3 are exact instantiations; <8, false> takes any
// d <= 8 at run time: its loops are unrolled to 8 with the columns >= d switched off (they read the centre and add zeros), so
// the 46 sums are named registers too (no scratch, tools/resource_report.sh; 44 fused multiply-adds per 64-byte row are far
// below the rate the row arrives at).  part[block][joint_fields(d)] in the compact layout of rsf_joint.h.
template <int D, bool EXACT>
__global__ void __launch_bounds__(kMaxBlock)
pool_joint_moments_kernel(int64_t n, int d, const double *__restrict__ x, JointCols A, double *__restrict__ part) {
  __shared__ double sh[kMaxBlock / 64][joint_fields(D)];
  double cnt = 0.0, bad = 0.0, s1[D], s2[D * (D + 1) / 2];
#pragma unroll
  for (int p = 0; p < D; ++p) s1[p] = 0.0;
#pragma unroll
  for (int e = 0; e < D * (D + 1) / 2; ++e) s2[e] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double v[D];
    bool ok = true;
#pragma unroll
    for (int p = 0; p < D; ++p) {
      const double xv = (EXACT || p < d) ? x[i * A.ld + A.col[p]] : A.c[p];
      ok = ok && __builtin_isfinite(xv);
      v[p] = xv - A.c[p];
    }
    cnt += ok ? 1.0 : 0.0;
    bad += ok ? 0.0 : 1.0;
#pragma unroll
    for (int p = 0; p < D; ++p) v[p] = ok ? v[p] : 0.0;  // a row with a non-finite entry adds zeros
    int e = 0;
#pragma unroll
    for (int p = 0; p < D; ++p) {
      s1[p] += v[p];
#pragma unroll
      for (int q = p; q < D; ++q, ++e) s2[e] = __builtin_fma(v[p], v[q], s2[e]);
    }
  }
  const int nd = EXACT ? D : d, wave = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
  auto emit = [&](double s, int f) {  // the wave's sum of s into field f of its LDS row
    s = wave_sum(s);
    if (lead) sh[wave][f] = s;
  };
  emit(cnt, 0);
  emit(bad, 1);
  int e = 0;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    if (EXACT || p < nd) emit(s1[p], RSF_JOINT_HEAD + p);
#pragma unroll
    for (int q = p; q < D; ++q, ++e)
      if (EXACT || q < nd) emit(s2[e], RSF_JOINT_HEAD + nd + p * nd - p * (p - 1) / 2 + (q - p));
  }
  __syncthreads();
  const int nf = joint_fields(nd);
  block_fields_store(sh, nf, part, (int64_t)blockIdx.x * nf);
}

// 2-D fixed-bin histogram (rsf_pool_histogram2d), pool_hist_kernel with a cell per pair of bins: one pass, HBM-bound, both
// columns of a row read by the same thread, LDS u32 counters, then 64-bit integer atomics into the global table for the
// non-empty cells.  Per axis the bin is hist_bin — numpy.histogramdd searches the same np.linspace edges.
struct Hist2dAxis {
  int32_t col, nbins;
  double lo, hi, scale, step;
};

__global__ void __launch_bounds__(kMaxBlock)
pool_hist2d_kernel(int64_t n, const double *__restrict__ x, int64_t ld, Hist2dAxis A, Hist2dAxis B, unsigned long long *__restrict__ counts) {
  extern __shared__ unsigned int hcells[];
  const int ncells = (A.nbins + 2) * (B.nbins + 2);
  for (int b = threadIdx.x; b < ncells; b += blockDim.x) hcells[b] = 0u;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int ba = hist_bin(x[i * ld + A.col], A.lo, A.hi, A.scale, A.step, A.nbins);
    const int bb = hist_bin(x[i * ld + B.col], B.lo, B.hi, B.scale, B.step, B.nbins);
    atomicAdd(&hcells[ba * (B.nbins + 2) + bb], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < ncells; b += blockDim.x)
    if (hcells[b]) atomicAdd(&counts[b], (unsigned long long)hcells[b]);
}

// 2-D Gaussian KDE (rsf_pool_kde2d): n m fp64 exp, bound by VALU issue.  The host factors H = L L^T and passes W = L^-1 / sqrt 2
// (lower triangular) and the centre c = the columns' means; with u = w00 (x_a - c_a), v = w10 (x_a - c_a) + w11 (x_b - c_b) the
// exponent of a pair is -(du^2 + dv^2).  Centring comes BEFORE scaling: Dc sits near 1000 with a spread of a few units.
// Points are whitened once by the thread that owns them, samples once as they enter the LDS tile — never per pair.  A thread
// keeps kKde2dPoints whitened points in registers, so one LDS broadcast read of (u, v), 16 bytes, serves that many pairs; per pair:
// two subtractions, a multiply, a fused multiply-add, rsf::fm::exp and an add.
// Grid: x = chunks of kMaxBlock * kKde2dPoints points, y = slices of the samples (a 64 x 64 mesh fills the part when n is small,
// 3e7 draws fill it when m is small).  partial[slice][m] is summed over the slices in index order by sum_in_order_kernel: the
// result depends on the inputs and on this geometry, which the host derives from (n, m) alone, and on nothing else.
// kKde2dPoints = 4, chosen by measurement among {1, 2, 4} (97.0, 100.4 and 95.3 ms for 33.6 M draws x 4096 points): DESIGN.md 4f.
constexpr int kKde2dPoints = 4;
constexpr int kKde2dChunk = kMaxBlock * kKde2dPoints;

struct Kde2dArgs {
  int64_t n, ld;
  int32_t ca, cb, m;
  double mean_a, mean_b, w00, w10, w11;
};

__global__ void __launch_bounds__(kMaxBlock)
pool_kde2d_kernel(Kde2dArgs A, const double *__restrict__ x, const double *__restrict__ points, double *__restrict__ partial) {
  __shared__ double2 tile[kKdeTile];
  const int64_t per = (A.n + gridDim.y - 1) / gridDim.y, lo = (int64_t)blockIdx.y * per, hi = min(A.n, lo + per);
  double pu[kKde2dPoints], pv[kKde2dPoints], acc[kKde2dPoints];
#pragma unroll
  for (int k = 0; k < kKde2dPoints; ++k) {
    const int64_t j = (int64_t)blockIdx.x * kKde2dChunk + k * kMaxBlock + threadIdx.x;
    const double da = j < A.m ? points[2 * j] - A.mean_a : 0.0, db = j < A.m ? points[2 * j + 1] - A.mean_b : 0.0;
    pu[k] = A.w00 * da;
    pv[k] = __builtin_fma(A.w10, da, A.w11 * db);
    acc[k] = 0.0;
  }
  for (int64_t t0 = lo; t0 < hi; t0 += kKdeTile) {
    const int tn = (int)min((int64_t)kKdeTile, hi - t0);
    __syncthreads();
    for (int t = threadIdx.x; t < tn; t += blockDim.x) {
      const double da = x[(t0 + t) * A.ld + A.ca] - A.mean_a, db = x[(t0 + t) * A.ld + A.cb] - A.mean_b;
      tile[t] = make_double2(A.w00 * da, __builtin_fma(A.w10, da, A.w11 * db));
    }
    __syncthreads();
    for (int t = 0; t < tn; ++t) {
      const double2 s = tile[t];
#pragma unroll
      for (int k = 0; k < kKde2dPoints; ++k) {
        const double du = pu[k] - s.x, dv = pv[k] - s.y;
        acc[k] += rsf::fm::exp(-__builtin_fma(dv, dv, du * du));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kKde2dPoints; ++k) {
    const int64_t j = (int64_t)blockIdx.x * kKde2dChunk + k * kMaxBlock + threadIdx.x;
    if (j < A.m) partial[(int64_t)blockIdx.y * A.m + j] = acc[k];
  }
}

}  // namespace rsfk
