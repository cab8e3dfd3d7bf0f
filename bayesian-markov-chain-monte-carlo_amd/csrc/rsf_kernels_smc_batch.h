// rsf_kernels_smc_batch.h — P independent populations of the tempered SMC sampler in one launch (include/rsf_smc_batch.h):
// smc_batch_init_kernel, smc_batch_max_kernel / _max_finish_kernel, smc_batch_weight_sums_kernel, smc_batch_tree_kernel,
// smc_batch_scan_tiles_kernel / _carry_kernel / _final_kernel, smc_batch_ancestor_kernel, smc_batch_gather_kernel,
// smc_batch_logtarget_kernel, smc_batch_move_kernel (the fused hot path), smc_batch_std2_kernel.  Included by rsf_smc.hip only,
// behind rsf_kernels_smc.h, whose chain logic (smc_proposal, smc_accept, smc_logtarget, smc_weight, smc_tile_chain, smc_count) it
// uses and does not restate.
//
// Geometry is the contract: blockIdx.x is what the single call derives from n, blockIdx.y is the population, and every sum keeps the
// single call's order within a population, so a population's bits are the single call's.  A workgroup belongs to one population:
// its parameters pops[blockIdx.y] are read at a wave-uniform address, and a workgroup of an inactive population returns before the
// first barrier.  No floating-point atomic; the accepted counts are 64-bit integer atomics, one per wave and step.
#pragma once
#include "../../include/rsf_smc_batch.h"
#include "rsf_kernels_smc.h"

namespace rsfk {

// what differs between the populations of a call; the box, the shape, n and the step count stay kernel arguments (SmcArgs)
struct SmcPop {
  uint64_t seed;
  int64_t offset;
  double beta, delta, lmax, u;  // lmax NaN (smc_batch_weight_sums_kernel only): the population's own, from its head
  double L[RSF_SMC_MAX_PARAMS * (RSF_SMC_MAX_PARAMS + 1) / 2];
  double dl[RSF_SMC_MAX_CANDIDATES];  // the candidates of the weight sums (unused ones 0, as SmcDeltas)
  uint32_t iter;
  int32_t group, active, pad_;
};

// the single call's argument block of this workgroup's population: the call's A with the population's stream, temperature and factor
__device__ __forceinline__ SmcArgs smc_pop_args(SmcArgs A, const SmcPop &P) {
  A.seed = P.seed; A.offset = P.offset; A.iter = P.iter; A.beta = P.beta;
#pragma unroll
  for (int k = 0; k < RSF_SMC_MAX_PARAMS * (RSF_SMC_MAX_PARAMS + 1) / 2; ++k) A.L[k] = P.L[k];
  return A;
}

// ---- the start: smc_init_kernel per population ------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(kMaxBlock) smc_batch_init_kernel(SmcArgs A0, const SmcPop *__restrict__ pops, double *__restrict__ q) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A0.n) return;
  const SmcArgs A = smc_pop_args(A0, pops[blockIdx.y]);
  q += (int64_t)blockIdx.y * A.n * D;
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

// ---- the weights' sums: smc_max_kernel, smc_max_finish_kernel, smc_weight_sums_kernel and the strided tree per population ----------
// part[population][block][kSmcHead]
__global__ void __launch_bounds__(kMaxBlock)
smc_batch_max_kernel(int64_t n, const SmcPop *__restrict__ pops, const double *__restrict__ l, double *__restrict__ part) {
  __shared__ double sh[kMaxBlock / 64][kSmcHead];
  if (!pops[blockIdx.y].active) return;
  l += (int64_t)blockIdx.y * n;
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
    for (int f = 0; f < kSmcHead; ++f) part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kSmcHead + f] = sh[0][f];
  }
}

// one workgroup per population: head[population][kSmcHead]
__global__ void __launch_bounds__(kMaxBlock)
smc_batch_max_finish_kernel(int nblocks, const SmcPop *__restrict__ pops, const double *__restrict__ part, double *__restrict__ head) {
  if (threadIdx.x != 0 || !pops[blockIdx.x].active) return;
  part += (int64_t)blockIdx.x * nblocks * kSmcHead;
  double m = -INFINITY, nf = 0.0, ni = 0.0;
  for (int b = 0; b < nblocks; ++b) { m = fmax(m, part[b * kSmcHead]); nf += part[b * kSmcHead + 1]; ni += part[b * kSmcHead + 2]; }
  head += blockIdx.x * kSmcHead;
  head[0] = m; head[1] = nf; head[2] = ni; head[3] = 0.0;
}

// part[population][block][kSmcFields]; lmax: the population's given constant, or its head's (the host refuses a head without one)
__global__ void __launch_bounds__(kMaxBlock) smc_batch_weight_sums_kernel(int64_t n, const SmcPop *__restrict__ pops, const double *__restrict__ l,
                                                                          const double *__restrict__ head, double *__restrict__ part) {
  __shared__ double sh[kMaxBlock / 64][kSmcFields];
  const SmcPop &P = pops[blockIdx.y];
  if (!P.active) return;
  l += (int64_t)blockIdx.y * n;
  const double lmax = P.lmax != P.lmax ? head[blockIdx.y * kSmcHead] : P.lmax;
  double s[kSmcFields];
#pragma unroll
  for (int f = 0; f < kSmcFields; ++f) s[f] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = l[i];
#pragma unroll
    for (int c = 0; c < RSF_SMC_MAX_CANDIDATES; ++c) {
      const double w = smc_weight(v, P.dl[c], lmax);
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
  block_fields_store(sh, kSmcFields, part, ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kSmcFields);
}

// rsfh::sum_strided_tree's order over each population's partials: out[population][nf], field f = blockIdx.x; thread t takes the
// partials t, t + 256, ... in that order from 0.0, then wave_sum and the waves in index order
__global__ void __launch_bounds__(kMaxBlock)
smc_batch_tree_kernel(int nblocks, int nf, const SmcPop *__restrict__ pops, const double *__restrict__ part, double *__restrict__ out) {
  __shared__ double sh[kMaxBlock / 64];
  if (!pops[blockIdx.y].active) return;
  part += (int64_t)blockIdx.y * nblocks * nf;
  const int f = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) s += part[(int64_t)b * nf + f];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (unsigned w = 1; w < blockDim.x / 64; ++w) s += sh[w];
    out[(int64_t)blockIdx.y * nf + f] = s;
  }
}

// ---- the prefix sum and the ancestors: the single call's kernels per population; tsum[population][ntiles] ------------------------
__global__ void __launch_bounds__(kMaxBlock)
smc_batch_scan_tiles_kernel(int64_t n, const SmcPop *__restrict__ pops, const double *__restrict__ l, double *__restrict__ tsum) {
  __shared__ double sh[kMaxBlock + 1];
  const SmcPop &P = pops[blockIdx.y];
  if (!P.active) return;
  double s[kSmcPerThread];
  (void)smc_tile_chain(n, l + (int64_t)blockIdx.y * n, P.delta, P.lmax, s, sh);
  if (threadIdx.x == 0) tsum[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[kMaxBlock];
}

__global__ void smc_batch_scan_carry_kernel(int64_t ntiles, const SmcPop *__restrict__ pops, double *__restrict__ tsum) {
  if (threadIdx.x != 0 || !pops[blockIdx.x].active) return;
  tsum += (int64_t)blockIdx.x * ntiles;
  double c = 0.0;
  for (int64_t b = 0; b < ntiles; ++b) {
    const double v = tsum[b];
    tsum[b] = c;
    c += v;
  }
}

__global__ void __launch_bounds__(kMaxBlock) smc_batch_scan_final_kernel(int64_t n, const SmcPop *__restrict__ pops, const double *__restrict__ l,
                                                                         const double *__restrict__ tcarry, double *__restrict__ cum) {
  __shared__ double sh[kMaxBlock + 1];
  const SmcPop &P = pops[blockIdx.y];
  if (!P.active) return;
  cum += (int64_t)blockIdx.y * n;
  double s[kSmcPerThread];
  const double ct = smc_tile_chain(n, l + (int64_t)blockIdx.y * n, P.delta, P.lmax, s, sh);
  const double cb = tcarry[(int64_t)blockIdx.y * gridDim.x + blockIdx.x];
  const int64_t base = (int64_t)blockIdx.x * kSmcTile + (int64_t)threadIdx.x * kSmcPerThread;
#pragma unroll
  for (int e = 0; e < kSmcPerThread; ++e)
    if (base + e < n) cum[base + e] = cb + (ct + s[e]);
}

// anc is local to the population: 0 .. n - 1
__global__ void __launch_bounds__(kMaxBlock)
smc_batch_ancestor_kernel(int64_t n, const SmcPop *__restrict__ pops, const double *__restrict__ cum, int64_t *__restrict__ anc) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const SmcPop &P = pops[blockIdx.y];
  if (j >= n || !P.active) return;
  cum += (int64_t)blockIdx.y * n;
  const double u = P.u;
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
  anc[(int64_t)blockIdx.y * n + j] = lo;
}

// an inactive population's particles are copied through (its anc is not read)
__global__ void __launch_bounds__(kMaxBlock)
smc_batch_gather_kernel(int64_t n, int d, const SmcPop *__restrict__ pops, const int64_t *__restrict__ anc, const double *__restrict__ q,
                        const double *__restrict__ l, double *__restrict__ q_out, double *__restrict__ l_out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t row = (int64_t)blockIdx.y * n;
  const int64_t a = pops[blockIdx.y].active ? anc[row + j] : j;
  for (int p = 0; p < d; ++p) q_out[(row + j) * d + p] = q[(row + a) * d + p];
  l_out[row + j] = l[row + a];
}

// ---- the solves --------------------------------------------------------------------------------------------------------------------
// the observation series of this workgroup's population (rsf::select_group, by the population's group index)
__device__ __forceinline__ void smc_select_group(Consts &K, const SmcPop &P) { K.data += (int64_t)P.group * K.nout; }

// The start's l = smc_logtarget(SSq) of particles inside the box (-inf outside): the fused path's solve, one launch for all
// populations.  As smc_move_kernel, a wave without a particle inside the box skips the solve and not the staging.
template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks)
smc_batch_logtarget_kernel(Consts K, SmcArgs A, const SmcPop *__restrict__ pops, const double *__restrict__ q, double *__restrict__ l) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  smc_select_group(K, pops[blockIdx.y]);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < A.n;
  const int64_t row = (int64_t)blockIdx.y * A.n + i;
  double x[D];
#pragma unroll
  for (int p = 0; p < D; ++p) x[p] = active ? q[row * D + p] : 0.5 * (A.lo[p] + A.hi[p]);
  const bool inb = active && in_box<D>(x, A);
  double pq[3] = {1000.0, K.a_def, K.b_def};
  if (inb) {
    pq[0] = x[0];
    if constexpr (D == 3) { pq[1] = x[1]; pq[2] = x[2]; }
  }
  const bool solve = __any(inb) != 0;  // wave-uniform
  const rsf::Lane L = rsf::make_lane<DAMP>(pq[0], pq[1], pq[2], K);
  rsf::State st = rsf::initial_state(pq[0], L, K);
  const double *ld = lds + rsf::lds_data_offset(K);
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
  if (active) l[row] = inb ? smc_logtarget(ssq, A.shape) : -INFINITY;
}

// The fused hot path: smc_move_kernel's step loop with the population's data row staged instead of the one series.  The staging
// barriers are the workgroup's and the workgroup is one population's, so an inactive population leaves before the first of them;
// cnt[population][step].
template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks)
smc_batch_move_kernel(Consts K, SmcArgs A0, const SmcPop *__restrict__ pops, double *__restrict__ q, double *__restrict__ l, unsigned long long *cnt) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const SmcPop &P = pops[blockIdx.y];
  if (!P.active) return;
  const SmcArgs A = smc_pop_args(A0, P);
  smc_select_group(K, P);
  q += (int64_t)blockIdx.y * A.n * D;
  l += (int64_t)blockIdx.y * A.n;
  cnt += (int64_t)blockIdx.y * A.steps;
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

// ---- the noise variance of the final particles: smc_std2_kernel per population ----------------------------------------------------------
__global__ void __launch_bounds__(kMaxBlock) smc_batch_std2_kernel(SmcArgs A0, const SmcPop *__restrict__ pops, double gd, double gc,
                                                                   const double *__restrict__ l, double *__restrict__ std2) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A0.n) return;
  const SmcArgs A = smc_pop_args(A0, pops[blockIdx.y]);
  const int64_t row = (int64_t)blockIdx.y * A.n + j;
  const double g = rsf::gamma_draw(A.seed, (uint64_t)(A.offset + j), A.iter, gd, gc);
  std2[row] = 0.5 * exp(-l[row] / A.shape) / g;
}

}  // namespace rsfk
