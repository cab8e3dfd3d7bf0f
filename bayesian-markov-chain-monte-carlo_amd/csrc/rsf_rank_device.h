// rsf_rank_device.h — the device functions of the order statistics that more than one unit uses: the order-preserving key
// of a double (rank_key, rank_value), np.quantile's pair and NumPy's _lerp (rank_pair, rank_lerp), and the radix select of a
// row's order statistics (rank_select), and the standard normal quantile (rank_ndtri).  No kernel: rsf_diag_rank.h (the rank
// kernels), rsf_predict.h (predict_select_kernel), rsf_psis.h (psis_row_kernel) and rsf_predict_noise.h (noise_quantile_row_kernel)
// include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsfk {

// ---- keys --------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t rank_key(double v) {
  uint64_t b = (uint64_t)__double_as_longlong(v);
  if (b == 0x8000000000000000ull) b = 0;  // -0.0 == +0.0
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double rank_value(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// Wichura's AS241 (PPND16): the standard normal quantile in float64, relative error about 1e-16.
__device__ double rank_ndtri(double p) {
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    return q * (((((((2.5090809287301226727e3 * r + 3.3430575583588128105e4) * r + 6.7265770927008700853e4) * r +
                    4.5921953931549871457e4) * r + 1.3731693765509461125e4) * r + 1.9715909503065514427e3) * r +
                 1.3314166789178437745e2) * r + 3.3871328727963666080e0) /
           (((((((5.2264952788528545610e3 * r + 2.8729085735721942674e4) * r + 3.9307895800092710610e4) * r +
                2.1213794301586595867e4) * r + 5.3941960214247511077e3) * r + 6.8718700749205790830e2) * r +
             4.2313330701600911252e1) * r + 1.0);
  }
  double r = q < 0.0 ? p : 1.0 - p;
  r = sqrt(-log(r));
  double z;
  if (r <= 5.0) {
    r -= 1.6;
    z = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
             1.27045825245236838258e0) * r + 3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r +
          4.63033784615654529590e0) * r + 1.42343711074968357734e0) /
        (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
             1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r +
          2.05319162663775882187e0) * r + 1.0);
  } else {
    r -= 5.0;
    z = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
             2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e0) * r +
          5.46378491116411436990e0) * r + 6.65790464350110377720e0) /
        (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
             7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
          5.99832206555887937690e-1) * r + 1.0);
  }
  return q < 0.0 ? -z : z;
}

// ---- order statistics ------------------------------------------------------------------------
// np.quantile(method="linear") of n sorted values at probability prob: the two order statistics it interpolates between
// (clamped to the ends) and the weight g of the upper one
__device__ __forceinline__ void rank_pair(int64_t n, double prob, int64_t &lo, int64_t &hi, double &g) {
#pragma clang fp contract(off)  // g is the rounded product minus its floor, as NumPy forms it
  const double h = (double)(n - 1) * prob;
  const double fl = floor(h);
  lo = (int64_t)fl;
  lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
  hi = lo + 1 < n ? lo + 1 : n - 1;
  g = h - fl;
}
// NumPy's _lerp
__device__ __forceinline__ double rank_lerp(double a, double b, double g) {
#pragma clang fp contract(off)  // bit for bit NumPy: no fused multiply-add
  const double diff = b - a;
  return g < 0.5 ? a + diff * g : b - diff * (1.0 - g);
}

// The MSD radix select of up to MAXR order statistics of one row of n keys, for a workgroup of 256 threads: eight passes of
// eight bits from the top, each a read of the row; per target rank a 256-bin histogram (LDS, integer atomics) of the keys that
// agree with the rank's prefix so far, then one thread per rank walks its bins to the digit that holds the rank.  Thread q < nr
// sets want[q] (the 0-based rank) before the call; after it prefix[q] is that order statistic's key.  key(j, pass): element j's.
// (The workgroup reductions of these files — diag_block_sum, psis_block_reduce, rank_block_scan, pred_sum8 — are NOT shared
// like this on purpose: each fixes its own summation order, and the order is part of the results' bits.  The orders that
// more than one kernel uses are the helpers of rsf_kernel_common.h.)
template <int MAXR>
struct RankSelect {
  uint32_t hist[MAXR][256];
  uint64_t prefix[MAXR];
  uint32_t want[MAXR];
};
template <int MAXR, typename KEY>
__device__ __forceinline__ void rank_select(RankSelect<MAXR> &S, int nr, int64_t n, KEY key) {
  const unsigned t = threadIdx.x;
  if (t < (unsigned)nr) S.prefix[t] = 0;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    const uint64_t mask = pass == 0 ? 0ull : ~0ull << (shift + 8);
    for (int e = t; e < nr * 256; e += 256) (&S.hist[0][0])[e] = 0;
    __syncthreads();
    const uint64_t pre = S.prefix[0];  // one rank: its prefix waits in a register (in pass 0 mask and prefix are both 0)
    for (int64_t j = t; j < n; j += 256) {
      const uint64_t k = key(j, pass);
      const unsigned dig = (unsigned)(k >> shift) & 255u;
      if constexpr (MAXR == 1) {
        if ((k & mask) == pre) atomicAdd(&S.hist[0][dig], 1u);
      } else if (pass == 0) {
        atomicAdd(&S.hist[0][dig], 1u);  // no prefix yet: every rank shares one histogram
      } else {
        for (int q = 0; q < nr; ++q)
          if ((k & mask) == S.prefix[q]) atomicAdd(&S.hist[q][dig], 1u);
      }
    }
    __syncthreads();
    if (t < (unsigned)nr) {
      const uint32_t *hq = S.hist[pass == 0 ? 0 : t];
      uint32_t below = 0, w = S.want[t];
      int dig = 0;
      for (; dig < 255; ++dig) {
        const uint32_t c = hq[dig];
        if (below + c > w) break;
        below += c;
      }
      S.want[t] = w - below;
      S.prefix[t] = (MAXR == 1 ? pre : S.prefix[t]) | (uint64_t)dig << shift;
    }
    __syncthreads();
  }
}

}  // namespace rsfk
