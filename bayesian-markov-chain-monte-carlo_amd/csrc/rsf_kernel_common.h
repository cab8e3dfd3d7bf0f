// rsf_kernel_common.h — what the kernel headers (rsf_kernels_core.h, rsf_kernels_sampler.h, rsf_kernels_pool.h, rsf_predict.h)
// and the host units (through rsf_host.h) share: constants, the sampler's argument block, the proposal's three device
// functions and the fixed-order sums over a wave's lanes and a workgroup's waves.  NO KERNEL lives here, so any unit may include it (a header that defines a non-template
// __global__ function belongs to exactly one unit).
//
// One lane = one chain, wave64 = 64 independent chains, fp64 VALU bound; no MFMA — the path is an elementwise ODE
// recurrence plus per-lane reductions, not a contraction:
//   forward_kernel  K1  batched RateStateModel.evaluate + SSq        (RateStateModel.py:188-395, MCMC.py:381-387)   rsf_kernels_core.h
//   init_kernel     K4  compute_initial_covariance + initial SSq     (MCMC.py:244-266, 468)                         rsf_kernels_core.h
//   mcmc_kernel     K2  n_iters fused Metropolis iterations          (MCMC.py:494-527)                              rsf_kernels_sampler.h
//   pool_*          posterior post-processing of the pooled draws    (RSF.py:717-746)                               rsf_kernels_pool.h
//   probe_*         K3  Philox / variate self-test entry points                                                     rsf_kernels_core.h
// The chain-independent tables (loading velocity V_l at the RK4 stage times, observation) are staged through LDS once per
// workgroup (or per chunk when they exceed the LDS budget) and read as wave-wide broadcasts; per-chain state lives in
// registers for the whole launch and touches HBM only at launch start/end plus one coalesced trace row per iteration.
//
// Per-chain state in HBM is STRUCTURE OF ARRAYS — q[p][C], V[e][C], window sums likewise — so that lane i of a wave reads
// element i of a contiguous 512-byte run whatever the number of parameters (the C ABI's [C][d] layout is transposed at
// rsf_mcmc_init / get_state / set_state, rsf_hip.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_abi.h"

namespace rsf { struct Consts; }  // rsf_device.h: the kernel headers include it, this one does not (host-only units see it)

namespace rsfk {

using rsf::Consts;

enum Mode : int { RK4_F64 = 0, RK4_F32 = 1, DOP853 = 2 };  // how the ODE is integrated (rsf_model.flags)

constexpr int kMaxBlock = 256;  // 4 waves: one per SIMD of a CU
// Register budget of the sampler kernels: at least this many workgroups per CU, i.e. waves per SIMD (2 => at most 256 of
// the 512 unified registers per lane).  cfg2 runs 4 waves per SIMD worth of chains, so a kernel that drifts above 256
// registers would run it in four rounds instead of two; the DOP853 sampler is held to the same budget (unbounded it took
// 300 registers and ran one wave per SIMD whatever the chain count: profiles/r02/dop853_occupancy_ab.log).
constexpr int kMinBlocks = 2;
// LDS per workgroup for the loading table + observation chunk.  Two workgroups per CU (kMinBlocks) at 56 KiB each fit the
// CU's 160 KiB next to the samplers' per-lane slots (up to 24 KiB: Cholesky factors, parked chain state); nsteps 2000
// (48 KB) stays resident for the whole launch instead of being staged twice per proposal (+1.3 % at cfg2).  The chunk LENGTH
// kc is sized for tables of doubles (rsf_set_model); the float32 SAMPLER, whose tables are floats, has its own (kc32: nsteps
// 4000 is one resident chunk of 48 KB there), the other float32 kernels share kc with the float64 init kernel of that mode.
constexpr size_t kLdsBudget = 56 * 1024;
// LDS slots (doubles) of a sampler launch behind the table chunk, per lane: d = 3: the Cholesky factor's six per chain; the
// float64 RK4 sampler adds the chain's point, sigma^2, SSq and log u parked across the forward solve (mcmc_kernel)
constexpr int factor_slots(int d) { return d == 3 ? 6 : 0; }
constexpr int park_slots(int d) { return factor_slots(d) + d + 3; }

// The accept test of MCMC.py:327-331: log alpha = clip(0.5 (SSq_prev - SSq_new) / sigma^2, -inf, 0) > log u.  np.clip keeps a
// NaN, and NaN > log u is False: a proposal whose series blew up (a stiff small-Dc lane under fixed-step RK4: Inf - Inf) is
// REJECTED.  fmin(x, 0) would not do: IEEE minNum returns the operand that is not NaN, i.e. 0 > log u, accepted — which is
// what this kernel did until round 4, unnoticed because no test before the wide-proposal ones produced a non-finite sum.
__device__ __forceinline__ bool accept_test(double ratio, double log_u) {
  const double logalpha = ratio > 0.0 ? 0.0 : ratio;  // NaN > 0 is false: NaN stays NaN
  return logalpha > log_u;                             // NaN compares false => reject
}

// The proposal of MCMC.py:497 from the chain's point, the lower Cholesky factor of its proposal covariance (row-major
// lower triangle, D (D + 1) / 2 entries) and D standard normals — one definition, so that rsf_mcmc_propose announces
// exactly the point the sampler kernels will evaluate.
template <int D, typename F>
__device__ __forceinline__ void propose(const double (&q)[D], F factor, const double *z, double (&qn)[D]) {
  int e = 0;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    double s = q[p];
#pragma unroll
    for (int r = 0; r <= p; ++r) s = __builtin_fma(factor(e++), z[r], s);
    qn[p] = s;
  }
}

// (ARGS: a kernel-argument struct with lo[] / hi[] members, indexed in place — a pointer INTO the argument block would make
// these per-lane flat loads, on the vector-memory counter the trace stores sit on, instead of scalar loads)
template <int D, typename ARGS>
__device__ __forceinline__ bool in_box(const double (&qn)[D], const ARGS &A) {
  bool inb = true;
#pragma unroll
  for (int p = 0; p < D; ++p) inb = inb && (qn[p] > A.lo[p]) && (qn[p] < A.hi[p]);  // strict box, MCMC.py:318-320
  return inb;
}

// ---- fixed-order sums over lanes and waves --------------------------------------------------------------------------
// The order of the additions is part of a result's bits: each helper below IS one order, and a reduction that adds in
// another order keeps its own code (pred_sum8, psis_block_reduce, the rank kernels' scans and min/max trees).

// descending shuffle tree, off = 32 .. 1: the wave's sum, valid in lane 0
template <class T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// ascending xor butterfly, s = 1 .. 32: the wave's sum (or maximum) in every lane (a + b == b + a bit for bit, so the lanes agree)
template <bool MAX> __device__ __forceinline__ double wave_all_ascending(double v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const double o = __shfl_xor(v, s, 64);
    v = MAX ? fmax(v, o) : v + o;
  }
  return v;
}

// descending xor butterfly, off = 32 .. 1: the wave's sum in every lane.  Not wave_all_ascending<false>: it pairs the lanes in
// the opposite sequence, which rounds differently
__device__ __forceinline__ double wave_all_descending(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The tail of a workgroup's per-field sums.  sh[w][f] is wave w's sum of field f, stored by its lead lane, and the caller's
// barrier lies between those stores and this call; thread f < nf (nf <= blockDim.x) adds the waves in index order from
// sh[0][f] and writes part[row + f], row = nf * the workgroup's index in part[block][nf].
template <int NF> __device__ __forceinline__ void block_fields_store(const double (*sh)[NF], int nf, double *part, int64_t row) {
  if (threadIdx.x < (unsigned)nf) {
    double s = sh[0][threadIdx.x];
    for (unsigned w = 1; w < blockDim.x / 64; ++w) s += sh[w][threadIdx.x];
    part[row + threadIdx.x] = s;
  }
}

struct McmcArgs {
  int64_t C, chain_offset, n_iters, iter_base;
  uint64_t seed;
  double n0, shape;
  double gd, gc;  // Marsaglia-Tsang constants of Gamma(shape): d = shape - 1/3, c = 1/sqrt(9 d)
  double lo[RSF_MAX_PARAMS], hi[RSF_MAX_PARAMS];
  int32_t adapt_mode, adapt_interval;
  int32_t lc_off;     // D = 3: offset (in doubles) of the per-lane Cholesky factors behind the table chunk in LDS
  double dict_scale;  // 2.38^2 / len(qpriors.keys()), MCMC.py:200 (reference_dict mode)
  double am_eps[RSF_MAX_PARAMS];  // am mode: (1e-6 (hi - lo))^2 added to the history's variances (rsf::window_covariance)
  double *q, *ssq, *std2, *V;           // per-chain state: q[d][C], ssq[C], std2[C], V[d*d][C]
  double *wref, *wsum, *wsq;            // adaptation window (shifted sums): [d][C], [d][C], [d*d][C]
  int32_t *wn;
  double *wbuf;                         // reference_dict: the window's samples themselves, [adapt_interval][C] (rsf::np_cov_1d)
  unsigned long long *stats;            // [RSF_CNT_COUNT] totals since rsf_mcmc_init (rsf_abi.h: rsf_mcmc_counters)
  const double *z, *u, *g;              // replay variates (REPLAY only): z[n][C][d], u[n][C], g[n][C]
  const double *ssq_new;                // INJECT only: the proposals' sums of squares, [n][C] (rsf_mcmc_replay_ssq)
  double *tq, *ts;                      // traces, iteration-major: tq[n][C][d] (the ABI's layout), ts[n][C]
  uint8_t *ta;
};

}  // namespace rsfk
