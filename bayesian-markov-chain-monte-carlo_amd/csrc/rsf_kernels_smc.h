// rsf_kernels_smc.h — tempered sequential Monte Carlo over the box prior (include/rsf_smc.h): smc_init_kernel, smc_max_kernel,
// smc_weight_sums_kernel, smc_scan_tiles_kernel / _carry_kernel / _final_kernel, smc_ancestor_kernel, smc_gather_kernel,
// smc_propose_kernel, smc_accept_kernel, smc_move_kernel (the fused hot path), smc_std2_kernel.  Included by rsf_smc.hip only.
// The last step of the weight sums, over the workgroups' partials, is rsfh::sum_strided_tree (rsf_host.h).
//
// Reproducibility: every sum below has an order fixed by the shape of the input and the launch geometry, which the host derives
// from n alone.  No floating-point atomic; the accepted counts are integers (64-bit integer atomics, order-free).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_smc.h"
#include "rsf_kernel_common.h"
#include "rsf_device.h"

namespace rsfk {

constexpr int kSmcBlocks = 1024;                        // workgroups of the weight kernels at most: four per CU
constexpr int kSmcFields = 2 * RSF_SMC_MAX_CANDIDATES;  // per candidate: sum w, sum w^2
constexpr int kSmcHead = 4;                             // largest finite l, finite entries, -inf entries, unused
constexpr int kSmcPerThread = 8;                        // consecutive weights a thread of the scan owns
constexpr int kSmcTile = kMaxBlock * kSmcPerThread;     // weights per tile of the scan
constexpr uint32_t kSmcSlotU2 = 3;                      // Philox slot of the third start coordinate's uniform (0..2: rsf_device.h)

// the box, the Philox key and the proposal factor of one call: a kernel argument, so that every entry is a scalar register
struct SmcArgs {
  int64_t n, offset;
  uint64_t seed;
  uint32_t iter;   // iteration of the first Metropolis step of the call (smc_init_kernel: 0)
  int32_t steps;
  double beta, shape;
  double L[RSF_SMC_MAX_PARAMS * (RSF_SMC_MAX_PARAMS + 1) / 2];  // row-major lower triangle
  double lo[RSF_SMC_MAX_PARAMS], hi[RSF_SMC_MAX_PARAMS];
};

// ---- the chain logic: ONE definition, used by the split kernels and by the fused one ----------------------------------------
// l = -shape log SSq; -inf where SSq is not finite or not positive
__device__ __forceinline__ double smc_logtarget(double ssq, double shape) {
  return (__builtin_isfinite(ssq) && ssq > 0.0) ? -shape * log(ssq) : -INFINITY;
}

// the proposal of (seed, particle gid, iteration it): q' = q + L z with the sampler's normals and its propose → inside the strict box?
template <int D>
__device__ __forceinline__ bool smc_proposal(const SmcArgs &A, uint64_t gid, uint32_t it, const double (&q)[D], double (&qn)[D]) {
  uint32_t w[4];
  double z[4] = {0, 0, 0, 0};
  rsf::draw_words(A.seed, gid, it, rsf::SLOT_Z01, w);
  rsf::normal_pair(w, z[0], z[1]);
  if (D > 2) { rsf::draw_words(A.seed, gid, it, rsf::SLOT_Z2, w); rsf::normal_pair(w, z[2], z[3]); }
  propose<D>(q, [&](int k) { return A.L[k]; }, z, qn);
  return in_box<D>(qn, A);
}

// accept when log u < beta (l' - l), u the sampler's accept uniform of (seed, gid, it); a non-finite l' is rejected (accept_test)
__device__ __forceinline__ bool smc_accept(const SmcArgs &A, uint64_t gid, uint32_t it, double l, double ln) {
  uint32_t w[4];
  rsf::draw_words(A.seed, gid, it, rsf::SLOT_U, w);
  return accept_test(A.beta * (ln - l), rsf::rng_log(rsf::u53(w[0], w[1])));
}

// the wave's accepted proposals into cnt[step]: one integer atomic per wave
__device__ __forceinline__ void smc_count(bool acc, unsigned long long *cnt) {
  const unsigned long long b = __ballot(acc);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(cnt, (unsigned long long)__popcll(b));
}

// ---- the start ------------------------------------------------------------------------------------------------------------
// q_p = lo_p + u_p (hi_p - lo_p), one fused multiply-add, u_0 and u_1 the two 53-bit uniforms of the accept slot's four words at
// iteration 0 (u_0 is the u of rsf_mcmc_draws), u_2 the first uniform of slot 3; a result that rounds onto an edge moves one ulp in
template <int D>
__global__ void __launch_bounds__(kMaxBlock) smc_init_kernel(SmcArgs A, double *__restrict__ q) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.n) return;
  uint32_t w[4];
  double u[3];
  rsf::draw_words(A.seed, (uint64_t)(A.offset + j), 0u, rsf::SLOT_U, w);
  u[0] = rsf::u53(w[0], w[1]);
  u[1] = rsf::u53(w[2], w[3]);
  if (D > 2) { rsf::draw_words(A.seed, (uint64_t)(A.offset + j), 0u, kSmcSlotU2, w); u[2] = rsf::u53(w[0], w[1]); }
#pragma unroll
  for (int p = 0; p < D; ++p) {
    double v = __builtin_fma(u[p], A.hi[p] - A.lo[p], A.lo[p]);
    if (!(v < A.hi[p])) v = nextafter(A.hi[p], A.lo[p]);
    if (!(v > A.lo[p])) v = nextafter(A.lo[p], A.hi[p]);
    q[j * D + p] = v;
  }
}

// ---- the weights' sums ------------------------------------------------------------------------------------------------------
// part[block][kSmcHead] = [largest finite l (-inf: none), finite entries, -inf entries, 0]; NaN and +inf are in neither count
__global__ void __launch_bounds__(kMaxBlock) smc_max_kernel(int64_t n, const double *__restrict__ l, double *__restrict__ part) {
  __shared__ double sh[kMaxBlock / 64][kSmcHead];
  double m = -INFINITY, nf = 0.0, ni = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = l[i];
    const bool fin = __builtin_isfinite(v);
    m = fin ? fmax(m, v) : m;
    nf += fin ? 1.0 : 0.0;
    ni += v == -INFINITY ? 1.0 : 0.0;
  }
  m = wave_all_ascending<true>(m);
  nf = wave_sum(nf);
  ni = wave_sum(ni);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[wave][0] = m; sh[wave][1] = nf; sh[wave][2] = ni; sh[wave][3] = 0.0; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (unsigned w = 1; w < blockDim.x / 64; ++w) { sh[0][0] = fmax(sh[0][0], sh[w][0]); sh[0][1] += sh[w][1]; sh[0][2] += sh[w][2]; }
    for (int f = 0; f < kSmcHead; ++f) part[(int64_t)blockIdx.x * kSmcHead + f] = sh[0][f];
  }
}

// one workgroup: the head of all blocks (the maximum is order-free, the counts are exact integers)
__global__ void __launch_bounds__(kMaxBlock) smc_max_finish_kernel(int nblocks, const double *__restrict__ part, double *__restrict__ head) {
  if (threadIdx.x != 0) return;
  double m = -INFINITY, nf = 0.0, ni = 0.0;
  for (int b = 0; b < nblocks; ++b) { m = fmax(m, part[b * kSmcHead]); nf += part[b * kSmcHead + 1]; ni += part[b * kSmcHead + 2]; }
  head[0] = m; head[1] = nf; head[2] = ni; head[3] = 0.0;
}

struct SmcDeltas { double v[RSF_SMC_MAX_CANDIDATES]; };

// the weight of one particle at the step delta: exp(delta (l - lmax)), 0 for l = -inf (also at delta = 0)
__device__ __forceinline__ double smc_weight(double l, double delta, double lmax) {
  return __builtin_isfinite(l) ? exp(delta * (l - lmax)) : 0.0;
}

// One read of l for all candidates: part[block][kSmcFields] = [sum w, sum w^2] per candidate (unused candidates carry delta = 0).
// Per thread in index order (stride gridDim.x blockDim.x), the wave's shuffle tree, the waves in index order.
__global__ void __launch_bounds__(kMaxBlock)
smc_weight_sums_kernel(int64_t n, const double *__restrict__ l, double lmax, SmcDeltas dl, double *__restrict__ part) {
  __shared__ double sh[kMaxBlock / 64][kSmcFields];
  double s[kSmcFields];
#pragma unroll
  for (int f = 0; f < kSmcFields; ++f) s[f] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = l[i];
#pragma unroll
    for (int c = 0; c < RSF_SMC_MAX_CANDIDATES; ++c) {
      const double w = smc_weight(v, dl.v[c], lmax);
      s[2 * c] += w;
      s[2 * c + 1] = __builtin_fma(w, w, s[2 * c + 1]);
    }
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int f = 0; f < kSmcFields; ++f) {
    const double v = wave_sum(s[f]);
    if ((threadIdx.x & 63) == 0) sh[wave][f] = v;
  }
  __syncthreads();
  block_fields_store(sh, kSmcFields, part, (int64_t)blockIdx.x * kSmcFields);
}

// ---- the inclusive prefix sum of the weights, and the ancestors -------------------------------------------------------------
// The order, which is the contract: a thread owns kSmcPerThread consecutive weights and adds them one by one from 0.0 (s_0 .. s_7);
// thread 0 of the workgroup adds the 256 thread totals of the tile one by one from 0.0 (the thread carries c_t); one thread adds
// the tile totals one by one from 0.0 (the tile carries C_b);  cum_i = C_b + (c_t + s_k).  Every carry IS the last prefix before it
// and rounding is monotone, so cum never decreases and a particle of weight 0 repeats its predecessor's value.
__device__ __forceinline__ double smc_tile_chain(int64_t n, const double *__restrict__ l, double delta, double lmax, double (&s)[kSmcPerThread],
                                                 double *sh) {
  const int64_t base = (int64_t)blockIdx.x * kSmcTile + (int64_t)threadIdx.x * kSmcPerThread;
  double run = 0.0;
#pragma unroll
  for (int e = 0; e < kSmcPerThread; ++e) {
    run += base + e < n ? smc_weight(l[base + e], delta, lmax) : 0.0;
    s[e] = run;
  }
  sh[threadIdx.x] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    double c = 0.0;
    for (int t = 0; t < kMaxBlock; ++t) {
      const double v = sh[t];
      sh[t] = c;
      c += v;
    }
    sh[kMaxBlock] = c;
  }
  __syncthreads();
  return sh[threadIdx.x];
}

__global__ void __launch_bounds__(kMaxBlock) smc_scan_tiles_kernel(int64_t n, const double *__restrict__ l, double delta, double lmax, double *__restrict__ tsum) {
  __shared__ double sh[kMaxBlock + 1];
  double s[kSmcPerThread];
  (void)smc_tile_chain(n, l, delta, lmax, s, sh);
  if (threadIdx.x == 0) tsum[blockIdx.x] = sh[kMaxBlock];
}

// the tile totals into the tile carries, in place, in index order
__global__ void smc_scan_carry_kernel(int64_t ntiles, double *__restrict__ tsum) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double c = 0.0;
  for (int64_t b = 0; b < ntiles; ++b) {
    const double v = tsum[b];
    tsum[b] = c;
    c += v;
  }
}

__global__ void __launch_bounds__(kMaxBlock)
smc_scan_final_kernel(int64_t n, const double *__restrict__ l, double delta, double lmax, const double *__restrict__ tcarry, double *__restrict__ cum) {
  __shared__ double sh[kMaxBlock + 1];
  double s[kSmcPerThread];
  const double ct = smc_tile_chain(n, l, delta, lmax, s, sh);
  const double cb = tcarry[blockIdx.x];
  const int64_t base = (int64_t)blockIdx.x * kSmcTile + (int64_t)threadIdx.x * kSmcPerThread;
#pragma unroll
  for (int e = 0; e < kSmcPerThread; ++e)
    if (base + e < n) cum[base + e] = cb + (ct + s[e]);
}

// Systematic resampling: offspring j takes t_j = ((j + u) W) / n, W = cum[n - 1], and the first i with cum_i > t_j, by bisection.
// t_j >= W (u = 1 and rounding): the first i with cum_i >= W, the last particle that carries weight.
__global__ void __launch_bounds__(kMaxBlock) smc_ancestor_kernel(int64_t n, const double *__restrict__ cum, double u, int64_t *__restrict__ anc) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const double W = cum[n - 1];
  const double t = (((double)j + u) * W) / (double)n;
  const bool past = !(t < W);
  int64_t lo = 0, hi = n - 1;  // the answer lies in [lo, hi]: cum[n - 1] = W satisfies either test
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const double c = cum[mid];
    if (past ? c >= W : c > t) hi = mid;
    else lo = mid + 1;
  }
  anc[j] = lo;
}

__global__ void __launch_bounds__(kMaxBlock) smc_gather_kernel(int64_t n, int d, const int64_t *__restrict__ anc, const double *__restrict__ q,
                                                               const double *__restrict__ l, double *__restrict__ q_out, double *__restrict__ l_out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t a = anc[j];
  for (int p = 0; p < d; ++p) q_out[j * d + p] = q[a * d + p];
  l_out[j] = l[a];
}

// ---- the Metropolis step, split in two for a caller that supplies SSq itself --------------------------------------------------
template <int D>
__global__ void __launch_bounds__(kMaxBlock) smc_propose_kernel(SmcArgs A, const double *__restrict__ q, double *__restrict__ qn, uint8_t *__restrict__ inbox) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.n) return;
  double x[D], xn[D];
#pragma unroll
  for (int p = 0; p < D; ++p) x[p] = q[j * D + p];
  inbox[j] = smc_proposal<D>(A, (uint64_t)(A.offset + j), A.iter, x, xn) ? 1 : 0;
#pragma unroll
  for (int p = 0; p < D; ++p) qn[j * D + p] = xn[p];
}

// ssq_new is read for the proposals inside the box only; cnt[0] counts the accepted
__global__ void __launch_bounds__(kMaxBlock)
smc_accept_kernel(SmcArgs A, int d, const double *__restrict__ qn, const uint8_t *__restrict__ inbox, const double *__restrict__ ssq_new,
                  double *__restrict__ q, double *__restrict__ l, unsigned long long *cnt) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool acc = false;
  if (j < A.n && inbox[j]) {
    const double ln = smc_logtarget(ssq_new[j], A.shape);
    acc = smc_accept(A, (uint64_t)(A.offset + j), A.iter, l[j], ln);
    if (acc) {
      for (int p = 0; p < d; ++p) q[j * d + p] = qn[j * d + p];
      l[j] = ln;
    }
  }
  smc_count(acc, cnt);
}

// ---- the fused hot path -------------------------------------------------------------------------------------------------------
// One lane per particle, A.steps Metropolis steps inside the launch; each step is a proposal, the box test and one float64 RK4
// solve driven by rsf::integrate_lockstep with the sum of squares against the observation kept per lane — the table and the
// observation staged chunk by chunk as evidence_logtarget_kernel stages them.  A lane outside the box, or past the last particle,
// rides along with a harmless point; a WAVE without a proposal inside the box skips the solve (it still takes part in the staging,
// whose barriers are the workgroup's).
template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) smc_move_kernel(Consts K, SmcArgs A, double *__restrict__ q, double *__restrict__ l,
                                                                        unsigned long long *cnt) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < A.n;
  const uint64_t gid = (uint64_t)(A.offset + i);
  double x[D], lx = active ? l[i] : 0.0;
#pragma unroll
  for (int p = 0; p < D; ++p) x[p] = active ? q[i * D + p] : 0.5 * (A.lo[p] + A.hi[p]);
  const double *ld = lds + rsf::lds_data_offset(K);
  for (int s = 0; s < A.steps; ++s) {
    double xn[D];
    const bool inb = smc_proposal<D>(A, gid, A.iter + (uint32_t)s, x, xn) && active;
    double pq[3] = {1000.0, K.a_def, K.b_def};
    if (inb) {
      pq[0] = xn[0];
      if constexpr (D == 3) { pq[1] = xn[1]; pq[2] = xn[2]; }
    }
    const bool solve = __any(inb) != 0;  // wave-uniform
    const rsf::Lane L = rsf::make_lane<DAMP>(pq[0], pq[1], pq[2], K);
    rsf::State st = rsf::initial_state(pq[0], L, K);
    double ssq = 0.0;
    for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
      const int kn = min(K.kc, K.nout - k0);
      rsf::stage_chunk(lds, K, k0, kn);
      if (k0 == 1) {  // sample 0 belongs to no chunk: acc[0] = 0, so the observation's square starts the sum
        const double d0 = lds[rsf::lds_d0_offset(K)];
        ssq = d0 * d0;
      }
      if (solve)
        rsf::integrate_lockstep<DAMP>(lds, K, L, st, kn, [&](double ak, int ko) { const double r = ak - ld[ko]; ssq = __builtin_fma(r, r, ssq); }, [] {});
    }
    const double ln = smc_logtarget(ssq, A.shape);
    const bool acc = inb && smc_accept(A, gid, A.iter + (uint32_t)s, lx, ln);
    if (acc) {
#pragma unroll
      for (int p = 0; p < D; ++p) x[p] = xn[p];
      lx = ln;
    }
    smc_count(acc, cnt + s);
  }
  if (active) {
#pragma unroll
    for (int p = 0; p < D; ++p) q[i * D + p] = x[p];
    l[i] = lx;
  }
}

// ---- the noise variance of the final particles --------------------------------------------------------------------------------
// sigma^2 | q ~ InvGamma(shape, SSq / 2), SSq = exp(-l / shape): 0.5 SSq / G with the sampler's gamma variate of (seed, gid, iter)
__global__ void __launch_bounds__(kMaxBlock) smc_std2_kernel(SmcArgs A, double gd, double gc, const double *__restrict__ l, double *__restrict__ std2) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.n) return;
  const double g = rsf::gamma_draw(A.seed, (uint64_t)(A.offset + j), A.iter, gd, gc);
  std2[j] = 0.5 * exp(-l[j] / A.shape) / g;
}

}  // namespace rsfk
