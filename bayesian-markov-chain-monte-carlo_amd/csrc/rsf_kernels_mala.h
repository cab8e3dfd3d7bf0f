// rsf_kernels_mala.h — Gauss-Newton manifold MALA (include/rsf_mala.h; tests/mala_reference.py is the specification):
// mala_propose / mala_decide, the iteration's two halves as device functions defined ONCE, the split kernels mala_propose_kernel /
// mala_accept_kernel around them and mala_kernel, the fused hot path on FitGroup's group solve.  Included by rsf_mala.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_mala.h"
#include "rsf_kernels_fit.h"

namespace rsfk {

struct MalaArgs {
  int64_t n, offset;
  int64_t group_chains;  // chains per observation series (0: one series for all)
  uint64_t seed;
  uint32_t iter;         // Philox iteration of the call's first iteration
  int32_t n_iter;
  double fd, eps, lam, shape;
  double lo[RSF_MALA_MAX_PARAMS], hi[RSF_MALA_MAX_PARAMS];
  double *q, *ssq, *grad, *jtj;          // [n][d], [n], [n][d], [n][d][d]
  int32_t *accepted, *outbox, *stuck;    // [n] each
  double *tq, *ts;                       // traces, iteration-major: tq[n_iter][n][d], ts[n_iter][n]; both NULL or both set
};

// what mala_propose found of a chain
enum MalaProposal : int { MALA_STUCK = 0, MALA_OUTSIDE = 1, MALA_INSIDE = 2 };

// ---- the metric's factor and its triangular solves, once ------------------------------------------------------------------------
// All of it is compiled WITHOUT contraction of a product and a sum into a fused multiply-add, as fit_trial is: every operation is
// the IEEE one the specification's NumPy takes, in the same order.
// A = H + lam diag(H) = L L^T in fit_trial's operation order (H: full row-major, its lower triangle is read); false: a pivot is not
// positive and finite.  ld = sum_p log L_pp.
template <int D>
__device__ __forceinline__ bool mala_factor(const double (&H)[D * D], double lam, double (&L)[D * D], double &ld) {
#pragma clang fp contract(off)
  bool ok = true;
#pragma unroll
  for (int p = 0; p < D; ++p) {
#pragma unroll
    for (int r = 0; r <= p; ++r) {
      double s = H[p * D + r];
      if (r == p) s += lam * s;
#pragma unroll
      for (int k = 0; k < r; ++k) s -= L[p * D + k] * L[r * D + k];
      if (r == p) {
        ok = ok && s > 0.0 && s < INFINITY;  // NaN compares false
        L[p * D + p] = sqrt(s);
      } else {
        L[p * D + r] = s / L[r * D + r];
      }
    }
  }
  ld = 0.0;
  if (ok) {
    ld = log(L[0]);
#pragma unroll
    for (int p = 1; p < D; ++p) ld += log(L[p * D + p]);
  }
  return ok;
}

// delta = -(L L^T)^-1 g: L y = -g, then L^T delta = y in place
template <int D>
__device__ __forceinline__ void mala_step(const double (&L)[D * D], const double (&g)[D], double (&y)[D]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int p = 0; p < D; ++p) {
    double s = -g[p];
#pragma unroll
    for (int k = 0; k < p; ++k) s -= L[p * D + k] * y[k];
    y[p] = s / L[p * D + p];
  }
#pragma unroll
  for (int p = D - 1; p >= 0; --p) {
    double s = y[p];
#pragma unroll
    for (int k = p + 1; k < D; ++k) s -= L[k * D + p] * y[k];
    y[p] = s / L[p * D + p];
  }
}

// the draws of (seed, chain gid, iteration it): rsf_mcmc_draws' z and the logarithm of its u
template <int D>
__device__ __forceinline__ void mala_draws(const MalaArgs &A, uint64_t gid, uint32_t it, double (&z)[D], double &log_u) {
  uint32_t w[4];
  double zz[4] = {0, 0, 0, 0};
  rsf::draw_words(A.seed, gid, it, rsf::SLOT_Z01, w);
  rsf::normal_pair(w, zz[0], zz[1]);
  if (D > 2) { rsf::draw_words(A.seed, gid, it, rsf::SLOT_Z2, w); rsf::normal_pair(w, zz[2], zz[3]); }
#pragma unroll
  for (int p = 0; p < D; ++p) z[p] = zz[p];
  rsf::draw_words(A.seed, gid, it, rsf::SLOT_U, w);
  log_u = rsf::rng_log(rsf::u53(w[0], w[1]));
}

// ---- the iteration's two halves -------------------------------------------------------------------------------------------------
// Propose, steps 1-4: qn (written unless the chain is stuck) and ld = sum log L_pp of the factor at q.
template <int D>
__device__ __forceinline__ int mala_propose(const double (&q)[D], double ssq, const double (&g)[D], const double (&H)[D * D], const double (&z)[D],
                                            const MalaArgs &A, double (&qn)[D], double &ld) {
#pragma clang fp contract(off)
  double L[D * D], y[D], w[D];
  const bool ok = mala_factor<D>(H, A.lam, L, ld);
  if (!(ok && ssq > 0.0 && ssq < INFINITY)) return MALA_STUCK;
  mala_step<D>(L, g, y);
#pragma unroll
  for (int p = D - 1; p >= 0; --p) {  // L^T w = z
    double s = z[p];
#pragma unroll
    for (int k = p + 1; k < D; ++k) s -= L[k * D + p] * w[k];
    w[p] = s / L[p * D + p];
  }
  const double s = A.eps * sqrt(ssq / (2.0 * A.shape)), h = 0.5 * (A.eps * A.eps);
#pragma unroll
  for (int p = 0; p < D; ++p) qn[p] = (q[p] + h * y[p]) + s * w[p];
  return in_box<D>(qn, A) ? MALA_INSIDE : MALA_OUTSIDE;
}

// Decide, steps 1-4, for a proposal INSIDE the box: (ssq_n, g_n, H_n) the normal equations at qn, ld and z the proposal's → accepted?
template <int D>
__device__ __forceinline__ bool mala_decide(const double (&q)[D], double ssq, double ld, const double (&z)[D], double log_u, const double (&qn)[D],
                                            double ssq_n, const double (&g_n)[D], const double (&H_n)[D * D], const MalaArgs &A) {
#pragma clang fp contract(off)
  double L[D * D], y[D], e[D], ld_n;
  const bool ok = mala_factor<D>(H_n, A.lam, L, ld_n);
  if (!(ok && ssq_n > 0.0 && ssq_n < INFINITY)) return false;
  mala_step<D>(L, g_n, y);
  const double eps2 = A.eps * A.eps, h = 0.5 * eps2;
  double zz = 0.0, vv = 0.0;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    e[p] = q[p] - (qn[p] + h * y[p]);
    zz += z[p] * z[p];
  }
#pragma unroll
  for (int p = 0; p < D; ++p) {  // v = L^T e
    double v = L[p * D + p] * e[p];
#pragma unroll
    for (int k = p + 1; k < D; ++k) v += L[k * D + p] * e[k];
    vv += v * v;
  }
  const double la = ((-(A.shape + 0.5 * D) * (log(ssq_n) - log(ssq)) + (ld_n - ld)) + 0.5 * zz) - (A.shape / (ssq_n * eps2)) * vv;
  return log_u < la;  // NaN compares false: rejected
}

// a chain's state from and to global memory
template <int D>
__device__ __forceinline__ void mala_load(const MalaArgs &A, int64_t i, double (&q)[D], double &ssq, double (&g)[D], double (&H)[D * D]) {
#pragma unroll
  for (int p = 0; p < D; ++p) { q[p] = A.q[i * D + p]; g[p] = A.grad[i * D + p]; }
#pragma unroll
  for (int e = 0; e < D * D; ++e) H[e] = A.jtj[i * D * D + e];
  ssq = A.ssq[i];
}
template <int D>
__device__ __forceinline__ void mala_store(const MalaArgs &A, int64_t i, const double (&q)[D], double ssq, const double (&g)[D], const double (&H)[D * D]) {
#pragma unroll
  for (int p = 0; p < D; ++p) { A.q[i * D + p] = q[p]; A.grad[i * D + p] = g[p]; }
#pragma unroll
  for (int e = 0; e < D * D; ++e) A.jtj[i * D * D + e] = H[e];
  A.ssq[i] = ssq;
}
// what one lane per chain writes after the decision: the counter that grows, if any
__device__ __forceinline__ void mala_count(const MalaArgs &A, int64_t i, int found, bool acc) {
  if (acc) A.accepted[i] += 1;
  else if (found == MALA_OUTSIDE) A.outbox[i] += 1;
  else if (found == MALA_STUCK) A.stuck[i] += 1;
}

// ---- the split kernels: one thread per chain ------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(kMaxBlock) mala_propose_kernel(MalaArgs A, double *__restrict__ q_new, uint8_t *__restrict__ inbox,
                                                                 uint8_t *__restrict__ stuck) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  double q[D], g[D], H[D * D], ssq, z[D], qn[D], log_u, ld;
  mala_load<D>(A, i, q, ssq, g, H);
  mala_draws<D>(A, (uint64_t)(A.offset + i), A.iter, z, log_u);
  const int found = mala_propose<D>(q, ssq, g, H, z, A, qn, ld);
#pragma unroll
  for (int p = 0; p < D; ++p) q_new[i * D + p] = found == MALA_INSIDE ? qn[p] : q[p];
  inbox[i] = found == MALA_INSIDE ? 1 : 0;
  stuck[i] = found == MALA_STUCK ? 1 : 0;
}

template <int D>
__global__ void __launch_bounds__(kMaxBlock)
mala_accept_kernel(MalaArgs A, const double *__restrict__ q_new, const uint8_t *__restrict__ inbox, const double *__restrict__ ssq_new,
                   const double *__restrict__ grad_new, const double *__restrict__ jtj_new) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  double q[D], g[D], H[D * D], ssq, z[D], qn[D], log_u, ld;
  mala_load<D>(A, i, q, ssq, g, H);
  mala_draws<D>(A, (uint64_t)(A.offset + i), A.iter, z, log_u);
  const int found = mala_propose<D>(q, ssq, g, H, z, A, qn, ld);  // the factor at q again: ld, and what became of the proposal
  bool acc = false;
  if (found == MALA_INSIDE && inbox[i] != 0) {
    double g_n[D], H_n[D * D];
    const double ssq_n = ssq_new[i];
#pragma unroll
    for (int p = 0; p < D; ++p) { qn[p] = q_new[i * D + p]; g_n[p] = grad_new[i * D + p]; }
#pragma unroll
    for (int e = 0; e < D * D; ++e) H_n[e] = jtj_new[i * D * D + e];
    acc = mala_decide<D>(q, ssq, ld, z, log_u, qn, ssq_n, g_n, H_n, A);
    if (acc) mala_store<D>(A, i, qn, ssq_n, g_n, H_n);
  }
  mala_count(A, i, found, acc);
}

// ---- the fused hot path -----------------------------------------------------------------------------------------------------------
// fit_kernel's arrangement on FitGroup's group solve.  A.n_iter iterations (workgroup-uniform) inside the launch.  Per iteration:
// every lane of a group reads its chain's state from global memory, draws z and forms the same proposal (mala_propose), the group
// solves there (the forward-difference neighbours in lanes 1..D), then every lane reads the state again, forms the proposal again,
// takes the same decision from the same sums (mala_decide) and stores the same values — so that across the solve only the sums
// and one flag are live (the registers are the solve's), and a lane only ever reads back what it stored itself.  A chain without
// a proposal inside the box rides along on its own point; a WAVE without one skips the solve but not the staging, whose barriers
// are the workgroup's.  The counters and the trace rows are the group's lane 0's.
template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) mala_kernel(Consts K, MalaArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  FitGroup<D> grp;
  grp.select_group(K, A.group_chains);
  const int64_t i = grp.start;
  const bool active = i < A.n;
  const uint64_t gid = (uint64_t)(A.offset + i);
  for (int it = 0; it < A.n_iter; ++it) {
    bool inside = false;
    double pq[3] = {1000.0, K.a_def, K.b_def}, inv_den;
    if (active) {
      double q[D], g[D], H[D * D], ssq, z[D], qn[D], log_u, ld;
      mala_load<D>(A, i, q, ssq, g, H);
      mala_draws<D>(A, gid, A.iter + (uint32_t)it, z, log_u);
      inside = mala_propose<D>(q, ssq, g, H, z, A, qn, ld) == MALA_INSIDE;
      pq[0] = inside ? qn[0] : q[0];
      if constexpr (D == 3) { pq[1] = inside ? qn[1] : q[1]; pq[2] = inside ? qn[2] : q[2]; }
    }
    grp.perturb(A.fd, pq, inv_den);
    grp.template solve_group<DAMP>(lds, K, pq, inv_den, __any(inside) != 0);
    if (active) {
      double q[D], g[D], H[D * D], ssq, z[D], qn[D], log_u, ld, H_n[D * D];
      mala_load<D>(A, i, q, ssq, g, H);
      mala_draws<D>(A, gid, A.iter + (uint32_t)it, z, log_u);
      const int found = mala_propose<D>(q, ssq, g, H, z, A, qn, ld);  // the point the group solved at, again
      grp.full(H_n);
      const bool acc = found == MALA_INSIDE && mala_decide<D>(q, ssq, ld, z, log_u, qn, grp.ssq, grp.xtr, H_n, A);
      if (acc) mala_store<D>(A, i, qn, grp.ssq, grp.xtr, H_n);
      if (grp.tr == 0) {
        mala_count(A, i, found, acc);
        if (A.tq) {
          const int64_t row = (int64_t)it * A.n + i;
#pragma unroll
          for (int p = 0; p < D; ++p) A.tq[row * D + p] = acc ? qn[p] : q[p];
          A.ts[row] = acc ? grp.ssq : ssq;
        }
      }
    }
  }
}

}  // namespace rsfk
