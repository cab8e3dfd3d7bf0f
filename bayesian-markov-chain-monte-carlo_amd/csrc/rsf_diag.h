// rsf_diag.h — convergence diagnostics of a kept trace x[n][C][d] (include/rsf_diag.h): the device passes that produce the
// additive partials of split R-hat, nested R-hat and the multi-chain ESS.  Included by rsf_diag.hip only; the host finish that
// turns the partials into the statistics is plain C++ there (rsf_diag_finish).
//
//   diag_chain_kernel   pass 1a: one lane per chain, all d parameters (a wave reads 64*d contiguous doubles per row).  Split
//                       halves (first N and last N draws, N = n/2) and the whole chain: means and centred sums of squares
//                       (two sweeps, so a chain that barely moves keeps its variance to rounding); per-chain results for the
//                       later passes and one deterministic partial per workgroup of sum(xbar_m - c), sum(xbar_m - c)^2,
//                       sum s2_m over the split chains.
//   diag_super_kernel   pass 1b: one wave per superchain of S consecutive chains: superchain mean, Btilde_k, Wtilde_k.
//   diag_lag_kernel     pass 2: centred lagged products A_sum(t) = sum_m acov_m(t) for a tile of kLagTile lags.  One lane per
//                       chain (both split halves), the series in registers: kLagTile accumulators, a block of kLagTile current
//                       draws and a window of 2*kLagTile lagged draws, all indexed by constants of unrolled loops (ScratchSize
//                       0).  A tile re-reads the trace twice; the tiles and parameters of one chain block are dispatched next
//                       to each other so that they stream the same rows through L2 together.
// The per-workgroup partials of all three are summed in index order by rsfh::sum_in_order (rsf_host.h): every reduction is
// deterministic, no float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsf_kernel_common.h"

namespace rsfk {

constexpr int kDiagBlock = 256;   // chains per workgroup in passes 1a and 2
constexpr int kDiagSuperBlocks = 1024;  // pass 1b: at most this many workgroups of 4 waves, grid-stride over superchains
constexpr int kLagTile = 16;      // lags per lane in pass 2: 16 accumulators + 16 current + 32 lagged draws = 128 VGPRs

// fields of the pass-1a workgroup partial, per parameter
constexpr int kDiagChainFields = 3;  // sum(xbar_m - c), sum(xbar_m - c)^2, sum s2_m
constexpr int kDiagSuperFields = 4;  // sum(xbar_k - c), sum(xbar_k - c)^2, sum Btilde_k, sum Wtilde_k

struct DiagCenter {
  double v[3];  // the caller's centre c[p] (by value: no device buffer for three numbers)
};

struct DiagShape {
  int64_t n, C;  // iterations, chains
  int d;         // parameters (1..3)
  int64_t N;     // split-chain length n/2
  int64_t off2;  // first row of the second half: n - N
};

// fixed-order workgroup sum of one double per thread; every thread gets the total (blockDim.x = kDiagBlock)
__device__ __forceinline__ double diag_block_sum(double v, double *sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
  for (unsigned w = 1; w < blockDim.x / 64; ++w) s += sh[w];
  return s;
}

// per chain c and parameter p: mh[h][p][C] split-half means, fm[p][C] / fv[p][C] whole-chain mean and variance (ddof 1);
// part[block][p][kDiagChainFields].  The parameters are the innermost loop, so that a wave reads each row's 64*D contiguous
// doubles once per sweep.
template <int D>
__global__ void __launch_bounds__(kDiagBlock)
diag_chain_kernel(DiagShape s, const double *__restrict__ x, DiagCenter center, double *__restrict__ mh,
                  double *__restrict__ fm, double *__restrict__ fv, double *__restrict__ part) {
  __shared__ double sh[kDiagBlock / 64];
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = c < s.C;
  const int64_t row = s.C * D;
  const double *xc = x + (live ? c : 0) * D;
  const double rN = 1.0 / (double)s.N, rN1 = 1.0 / (double)(s.N - 1);
  double m0[D], m1[D], ss0[D], ss1[D];
  for (int p = 0; p < D; ++p) { m0[p] = m1[p] = ss0[p] = ss1[p] = 0.0; }
  if (live) {
    // sweep 1: means about the chain's first draw
    double x0[D], a0[D], a1[D];
#pragma unroll
    for (int p = 0; p < D; ++p) { x0[p] = xc[p]; a0[p] = a1[p] = 0.0; }
    for (int64_t i = 0; i < s.N; ++i) {
#pragma unroll
      for (int p = 0; p < D; ++p) {
        a0[p] += xc[i * row + p] - x0[p];
        a1[p] += xc[(s.off2 + i) * row + p] - x0[p];
      }
    }
    double e0[D], e1[D];
#pragma unroll
    for (int p = 0; p < D; ++p) { m0[p] = x0[p] + a0[p] * rN; m1[p] = x0[p] + a1[p] * rN; e0[p] = e1[p] = 0.0; }
    // sweep 2: centred sums of squares, with the corrected two-pass term (sum of residuals)^2 / N
    for (int64_t i = 0; i < s.N; ++i) {
#pragma unroll
      for (int p = 0; p < D; ++p) {
        const double r0 = xc[i * row + p] - m0[p], r1 = xc[(s.off2 + i) * row + p] - m1[p];
        e0[p] += r0; ss0[p] = __builtin_fma(r0, r0, ss0[p]);
        e1[p] += r1; ss1[p] = __builtin_fma(r1, r1, ss1[p]);
      }
    }
    // the whole chain (middle draw included when n is odd) by the pairwise combination of the halves
    const double n = (double)s.n;
    const bool odd = s.off2 != s.N;
#pragma unroll
    for (int p = 0; p < D; ++p) {
      ss0[p] -= e0[p] * e0[p] * rN;
      ss1[p] -= e1[p] * e1[p] * rN;
      const double xm = odd ? xc[s.N * row + p] : 0.0;
      const double fmean = ((double)s.N * (m0[p] + m1[p]) + xm) / n;
      const double d0 = m0[p] - fmean, d1 = m1[p] - fmean, dm = xm - fmean;
      mh[(int64_t)p * s.C + c] = m0[p];
      mh[((int64_t)D + p) * s.C + c] = m1[p];
      fm[(int64_t)p * s.C + c] = fmean;
      fv[(int64_t)p * s.C + c] = (ss0[p] + ss1[p] + (double)s.N * (d0 * d0 + d1 * d1) + (odd ? dm * dm : 0.0)) / (n - 1.0);
    }
  }
  for (int p = 0; p < D; ++p) {
    const double cp = center.v[p];
    const double y0 = live ? m0[p] - cp : 0.0, y1 = live ? m1[p] - cp : 0.0;
    const double f0 = diag_block_sum(y0 + y1, sh);
    const double f1 = diag_block_sum(y0 * y0 + y1 * y1, sh);
    const double f2 = diag_block_sum(live ? ss0[p] * rN1 + ss1[p] * rN1 : 0.0, sh);
    if (threadIdx.x == 0) {
      double *o = part + ((int64_t)blockIdx.x * D + p) * kDiagChainFields;
      o[0] = f0; o[1] = f1; o[2] = f2;
    }
  }
}

// one wave per superchain k of S chains [kS, (k+1)S): xbar_k - c, Btilde_k (ddof 1 over the chain means; 0 when S = 1) and
// Wtilde_k (mean of the chains' variances).  Each wave sums its superchains in a fixed order, the workgroup its waves in a
// fixed order: part[block][p][kDiagSuperFields]
__global__ void __launch_bounds__(kDiagBlock)
diag_super_kernel(int64_t C, int d, int64_t S, DiagCenter center, const double *__restrict__ fm,
                  const double *__restrict__ fv, double *__restrict__ part) {
  __shared__ double sh[kDiagBlock / 64][kDiagSuperFields];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t K = C / S;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / 64);
  const double rS = 1.0 / (double)S;
  for (int p = 0; p < d; ++p) {
    const double cp = center.v[p];
    const double *m = fm + (int64_t)p * C, *v = fv + (int64_t)p * C;
    double acc[kDiagSuperFields] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k = (int64_t)blockIdx.x * (blockDim.x / 64) + wave; k < K; k += waves) {
      const int64_t c0 = k * S;
      double sm = 0.0, sv = 0.0;
      for (int64_t j = lane; j < S; j += 64) { sm += m[c0 + j] - cp; sv += v[c0 + j]; }
      sm = wave_all_descending(sm); sv = wave_all_descending(sv);
      const double yk = sm * rS;  // xbar_k - c, identical in every lane (butterfly)
      double sb = 0.0, eb = 0.0;
      for (int64_t j = lane; j < S; j += 64) {
        const double r = (m[c0 + j] - cp) - yk;
        eb += r; sb = __builtin_fma(r, r, sb);
      }
      sb = wave_all_descending(sb); eb = wave_all_descending(eb);
      const double bt = S > 1 ? (sb - eb * eb * rS) / (double)(S - 1) : 0.0;
      acc[0] += yk; acc[1] += yk * yk; acc[2] += bt; acc[3] += sv * rS;
    }
    __syncthreads();
    if (lane == 0)
      for (int f = 0; f < kDiagSuperFields; ++f) sh[wave][f] = acc[f];
    __syncthreads();
    block_fields_store(sh, kDiagSuperFields, part, ((int64_t)blockIdx.x * d + p) * kDiagSuperFields);
  }
}

// Y(i) of split half h of chain c, parameter p: the draw centred on its half's mean, 0 past the end of the half
__device__ __forceinline__ double diag_y(const double *__restrict__ xc, int64_t row, int64_t base, int64_t i, int64_t N, double m) {
  return i < N ? xc[(base + i) * row] - m : 0.0;
}

// Lags [lag0 + tile*kLagTile, + kLagTile) of every split chain of a block of chains, parameter p: A_sum per workgroup,
// part[cblock][p][L] for the L = lag_end - lag0 lags of the call.  Work item b: tile and parameter vary fastest, then the chain
// block — the tiles and parameters of one chain block run side by side and share the rows they read in L2.
__global__ void __launch_bounds__(kDiagBlock)
diag_lag_kernel(DiagShape s, const double *__restrict__ x, const double *__restrict__ mh, int64_t lag0, int64_t lag_end,
                double *__restrict__ part) {
  __shared__ double sh[kDiagBlock / 64];
  const int64_t L = lag_end - lag0;
  const int ntiles = (int)((L + kLagTile - 1) / kLagTile);
  const int tile = blockIdx.x % ntiles;
  const int p = (blockIdx.x / ntiles) % s.d;
  const int64_t cblock = blockIdx.x / ((int64_t)ntiles * s.d);
  const int64_t c = cblock * blockDim.x + threadIdx.x;
  const bool live = c < s.C;
  const int64_t t0 = lag0 + (int64_t)tile * kLagTile;
  const int64_t row = s.C * s.d;
  const double *xc = x + (live ? c : 0) * s.d + p;
  double acc[kLagTile];
#pragma unroll
  for (int j = 0; j < kLagTile; ++j) acc[j] = 0.0;
  if (live) {
    for (int h = 0; h < 2; ++h) {
      const int64_t base = h ? s.off2 : 0;
      const double m = mh[((int64_t)h * s.d + p) * s.C + c];
      double win[2 * kLagTile];
#pragma unroll
      for (int k = 0; k < kLagTile; ++k) win[k] = diag_y(xc, row, base, t0 + k, s.N, m);
      // the last draw that pairs with anything at lag t0 is N - 1 - t0
      for (int64_t i0 = 0; i0 < s.N - t0; i0 += kLagTile) {
        double cur[kLagTile];
#pragma unroll
        for (int k = 0; k < kLagTile; ++k) {
          cur[k] = diag_y(xc, row, base, i0 + k, s.N, m);
          win[kLagTile + k] = diag_y(xc, row, base, i0 + t0 + kLagTile + k, s.N, m);
        }
#pragma unroll
        for (int k = 0; k < kLagTile; ++k)
#pragma unroll
          for (int j = 0; j < kLagTile; ++j) acc[j] = __builtin_fma(cur[k], win[k + j], acc[j]);
#pragma unroll
        for (int k = 0; k < kLagTile; ++k) win[k] = win[kLagTile + k];
      }
    }
  }
  const double rN = 1.0 / (double)s.N;
  for (int j = 0; j < kLagTile; ++j) {
    const double t = diag_block_sum(acc[j] * rN, sh);  // acov_m(t) = (1/N) sum_i y_i y_(i+t), summed over the block's chains
    if (threadIdx.x == 0 && t0 + j < lag_end) part[(cblock * s.d + p) * L + (t0 - lag0) + j] = t;
  }
}

}  // namespace rsfk
