// rsf_kernels_fit.h — multi-start Levenberg-Marquardt least squares (include/rsf_fit.h; tests/fit_reference.py is the
// specification): fit_trial / fit_decide, the iteration's two halves as device functions defined ONCE, the split kernels
// fit_trial_kernel / fit_decide_kernel around them, fit_normal_kernel (the normal equations at a point) and fit_kernel, the fused
// hot path.  Included by rsf_fit.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_fit.h"
#include "rsf_kernel_common.h"
#include "rsf_device.h"

namespace rsfk {

struct FitArgs {
  int64_t n;
  int64_t group_starts;  // starts per observation series (0: one series for all)
  double fd, ftol;
  double lo[RSF_FIT_MAX_PARAMS], hi[RSF_FIT_MAX_PARAMS];
  int32_t n_iter;
  double *q, *ssq, *grad, *jtj, *lam;  // [n][d], [n], [n][d], [n][d][d], [n]
  int32_t *status, *iters;             // [n], [n]
};

// ---- the iteration's two halves ---------------------------------------------------------------------------------------------------
// Both are compiled WITHOUT contraction of a product and a sum into a fused multiply-add: every operation is then the IEEE one the
// specification's NumPy takes, in the same order, so the trial point and the decision do not depend on what the compiler fuses.
// Steps 1-2: A = H + lam diag(H) = L L^T (H: full row-major, its lower triangle is read), delta = -A^-1 g, qt = q + delta clamped
// into the strict box.  false: a pivot is not positive and finite, qt is not written.
template <int D, typename ARGS>
__device__ __forceinline__ bool fit_trial(const double (&q)[D], const double (&g)[D], const double (&H)[D * D], double lam, const ARGS &A,
                                          double (&qt)[D]) {
#pragma clang fp contract(off)
  double L[D * D], y[D];
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
  if (!ok) return false;
#pragma unroll
  for (int p = 0; p < D; ++p) {  // L y = -g
    double s = -g[p];
#pragma unroll
    for (int k = 0; k < p; ++k) s -= L[p * D + k] * y[k];
    y[p] = s / L[p * D + p];
  }
#pragma unroll
  for (int p = D - 1; p >= 0; --p) {  // L^T delta = y, in place
    double s = y[p];
#pragma unroll
    for (int k = p + 1; k < D; ++k) s -= L[k * D + p] * y[k];
    y[p] = s / L[p * D + p];
  }
#pragma unroll
  for (int p = 0; p < D; ++p) {
    double v = q[p] + y[p];
    if (v <= A.lo[p]) v = nextafter(A.lo[p], A.hi[p]);
    else if (v >= A.hi[p]) v = nextafter(A.hi[p], A.lo[p]);
    qt[p] = v;
  }
  return true;
}

// what fit_decide changes of a start
enum FitChange : int { FIT_REJECTED = 0, FIT_ACCEPTED = 1 };

// Steps 4-7 for a RUNNING start: ok = fit_trial's, (ssq_n, g_n, H_n) the normal equations at qt (read when ok).  Accepted: the
// caller's (q, ssq, g, H) become the trial's.  lam, status and iters change either way.
template <int D>
__device__ __forceinline__ int fit_decide(double (&q)[D], double &ssq, double (&g)[D], double (&H)[D * D], double &lam, int32_t &status,
                                          int32_t &iters, bool ok, const double (&qt)[D], double ssq_n, const double (&g_n)[D],
                                          const double (&H_n)[D * D], double ftol) {
#pragma clang fp contract(off)
  const bool acc = ok && ssq_n < INFINITY && ssq_n > -INFINITY && ssq_n < ssq;  // a NaN sum compares false: rejected
  iters += 1;
  if (acc) {
    if ((ssq - ssq_n) / ssq < ftol) status = RSF_FIT_CONVERGED;
#pragma unroll
    for (int p = 0; p < D; ++p) { q[p] = qt[p]; g[p] = g_n[p]; }
#pragma unroll
    for (int e = 0; e < D * D; ++e) H[e] = H_n[e];
    ssq = ssq_n;
    lam = fmax(RSF_FIT_LAM_DOWN * lam, RSF_FIT_LAM_MIN);
    return FIT_ACCEPTED;
  }
  lam = RSF_FIT_LAM_UP * lam;
  if (lam > RSF_FIT_LAM_MAX) status = RSF_FIT_STALLED;
  return FIT_REJECTED;
}

// a start's state from and to global memory
template <int D>
__device__ __forceinline__ void fit_load(const FitArgs &A, int64_t i, double (&q)[D], double (&g)[D], double (&H)[D * D], double &lam) {
#pragma unroll
  for (int p = 0; p < D; ++p) { q[p] = A.q[i * D + p]; g[p] = A.grad[i * D + p]; }
#pragma unroll
  for (int e = 0; e < D * D; ++e) H[e] = A.jtj[i * D * D + e];
  lam = A.lam[i];
}
template <int D>
__device__ __forceinline__ void fit_store(const FitArgs &A, int64_t i, int change, const double (&q)[D], double ssq, const double (&g)[D],
                                          const double (&H)[D * D], double lam, int32_t status, int32_t iters) {
  if (change == FIT_ACCEPTED) {
#pragma unroll
    for (int p = 0; p < D; ++p) { A.q[i * D + p] = q[p]; A.grad[i * D + p] = g[p]; }
#pragma unroll
    for (int e = 0; e < D * D; ++e) A.jtj[i * D * D + e] = H[e];
    A.ssq[i] = ssq;
  }
  A.lam[i] = lam;
  A.status[i] = status;
  A.iters[i] = iters;
}

// ---- the split kernels: one thread per start ------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(kMaxBlock) fit_trial_kernel(FitArgs A, double *__restrict__ q_trial, uint8_t *__restrict__ okv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  double q[D], g[D], H[D * D], lam, qt[D];
  fit_load<D>(A, i, q, g, H, lam);
  const bool ok = A.status[i] == RSF_FIT_RUNNING && fit_trial<D>(q, g, H, lam, A, qt);
#pragma unroll
  for (int p = 0; p < D; ++p) q_trial[i * D + p] = ok ? qt[p] : q[p];
  okv[i] = ok ? 1 : 0;
}

template <int D>
__global__ void __launch_bounds__(kMaxBlock)
fit_decide_kernel(FitArgs A, const double *__restrict__ q_trial, const uint8_t *__restrict__ okv, const double *__restrict__ ssq_new,
                  const double *__restrict__ grad_new, const double *__restrict__ jtj_new) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  int32_t status = A.status[i], iters = A.iters[i];
  if (status != RSF_FIT_RUNNING) return;
  double q[D], g[D], H[D * D], lam, ssq = A.ssq[i];
  fit_load<D>(A, i, q, g, H, lam);
  const bool ok = okv[i] != 0;
  double qt[D], g_n[D], H_n[D * D], ssq_n = 0.0;
#pragma unroll
  for (int p = 0; p < D; ++p) { qt[p] = q_trial[i * D + p]; g_n[p] = ok ? grad_new[i * D + p] : 0.0; }
#pragma unroll
  for (int e = 0; e < D * D; ++e) H_n[e] = ok ? jtj_new[i * D * D + e] : 0.0;
  if (ok) ssq_n = ssq_new[i];
  const int change = fit_decide<D>(q, ssq, g, H, lam, status, iters, ok, qt, ssq_n, g_n, H_n, A.ftol);
  fit_store<D>(A, i, change, q, ssq, g, H, lam, status, iters);
}

// ---- the normal equations of a group solve ----------------------------------------------------------------------------------------
// init_kernel's scheme (rsf_kernels_core.h, InitGroup; restated, that kernel's code stays as it is) with X^T r added: a start owns
// G = D + 1 adjacent lanes, lane 0 integrates the point, lane p + 1 the point with parameter p times (1 + fd); where an output
// sample completes the lanes exchange their acceleration samples by DPP quad_perm moves.  Unlike InitGroup EVERY lane of the group
// accumulates the start's sums, from lane 0's sample and the group's sensitivities: the same values in the same order, so the
// group's lanes hold the same bits and each can take the decision (fit_kernel) without a further exchange.
template <int D>
struct FitGroup {
  static constexpr int G = D + 1;  // lanes per start: 2 or 4, a power of two, so a group never straddles a wave
  const unsigned t = threadIdx.x;
  const int tr = (int)(t & (G - 1));  // which trajectory of its start this lane integrates
  const int64_t start = (int64_t)blockIdx.x * (blockDim.x / G) + (t / G);
  double xtx[D * D], xtr[D], ssq;

  // the observation series of the workgroup's starts (all of a workgroup's starts belong to one series)
  __device__ __forceinline__ void select_group(Consts &K, int64_t group_starts) const {
    if (group_starts > 0) K.data += (((int64_t)blockIdx.x * (blockDim.x / G)) / group_starts) * K.nout;
  }
  // this lane's parameter vector (Dc, a, b) from the start's point and, for a perturbed trajectory, 1 / (perturbed value * step)
  __device__ __forceinline__ void perturb(double fd, double (&pq)[3], double &inv_den) const {
    inv_den = 0.0;
#pragma unroll
    for (int p = 0; p < D; ++p)
      if (tr == p + 1) {
        pq[p] = pq[p] * (1 + fd);
        inv_den = 1.0 / (pq[p] * fd);
      }
  }
  // sample 0 belongs to no chunk: acc[0] = 0 in every trajectory, so the observation's square starts ssq and nothing else
  __device__ __forceinline__ void reset(double d0) {
    ssq = d0 * d0;
#pragma unroll
    for (int p = 0; p < D; ++p) xtr[p] = 0.0;
#pragma unroll
    for (int e = 0; e < D * D; ++e) xtx[e] = 0.0;
  }
  template <int SRC>
  static __device__ __forceinline__ double from_lane(double v) {
    return rsf::dpp_move<G == 4 ? (SRC | SRC << 2 | SRC << 4 | SRC << 6) : (SRC | SRC << 2 | (2 + SRC) << 4 | (2 + SRC) << 6)>(v);
  }
  template <int P>
  __device__ __forceinline__ void gather(double x, double (&xs)[D]) const {
    if constexpr (P < D) {
      xs[P] = from_lane<P + 1>(x);
      gather<P + 1>(x, xs);
    }
  }
  // an output sample is complete (every lane of the group calls, in converged control flow); the upper triangle of X^T X
  __device__ __forceinline__ void sample(double ak, double obs, double inv_den) {
    const double ak0 = from_lane<0>(ak);
    const double x = (ak - ak0) * inv_den;  // lane p + 1: the sensitivity to parameter p; lane 0: 0
    double xs[D];
    gather<0>(x, xs);
    const double r = ak0 - obs;
    ssq = __builtin_fma(r, r, ssq);
#pragma unroll
    for (int p = 0; p < D; ++p) {
      xtr[p] = __builtin_fma(xs[p], r, xtr[p]);
#pragma unroll
      for (int r2 = p; r2 < D; ++r2) xtx[p * D + r2] = __builtin_fma(xs[p], xs[r2], xtx[p * D + r2]);
    }
  }
  __device__ __forceinline__ void full(double (&H)[D * D]) const {
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
      for (int r2 = 0; r2 < D; ++r2) H[p * D + r2] = xtx[p <= r2 ? p * D + r2 : r2 * D + p];
  }
  // the group solve at the point pq (this lane's, perturbed): every thread of the workgroup calls (the staging's barriers);
  // a wave with solve == false takes part in the staging only
  template <bool DAMP>
  __device__ __forceinline__ void solve_group(double *lds, const Consts &K, const double (&pq)[3], double inv_den, bool solve) {
    const rsf::Lane L = rsf::make_lane<DAMP>(pq[0], pq[1], pq[2], K);
    rsf::State st = rsf::initial_state(pq[0], L, K);
    const double *ld = lds + rsf::lds_data_offset(K);
    for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
      const int kn = min(K.kc, K.nout - k0);
      rsf::stage_chunk(lds, K, k0, kn);
      if (k0 == 1) reset(lds[rsf::lds_d0_offset(K)]);
      if (solve) rsf::integrate_lockstep<DAMP>(lds, K, L, st, kn, [&](double ak, int ko) { sample(ak, ld[ko], inv_den); }, [] {});
    }
  }
};

template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) fit_normal_kernel(Consts K, FitArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  FitGroup<D> grp;
  grp.select_group(K, A.group_starts);
  const int64_t i = grp.start;
  const bool active = i < A.n;
  double pq[3] = {1000.0, K.a_def, K.b_def}, inv_den;
  if (active) {
    pq[0] = A.q[i * D];
    if constexpr (D == 3) { pq[1] = A.q[i * D + 1]; pq[2] = A.q[i * D + 2]; }
  }
  grp.perturb(A.fd, pq, inv_den);
  grp.template solve_group<DAMP>(lds, K, pq, inv_den, true);
  if (active && grp.tr == 0) {
    double H[D * D];
    grp.full(H);
    A.ssq[i] = grp.ssq;
#pragma unroll
    for (int p = 0; p < D; ++p) A.grad[i * D + p] = grp.xtr[p];
#pragma unroll
    for (int e = 0; e < D * D; ++e) A.jtj[i * D * D + e] = H[e];
  }
}

// ---- the fused hot path -----------------------------------------------------------------------------------------------------------
// A.n_iter iterations (workgroup-uniform) inside the launch.  Per iteration: every lane of a group reads its start's state from
// global memory and forms the same trial point (fit_trial), the group solves there, then every lane reads the state again, takes
// the same decision from the same sums (fit_decide) and stores the same values — so that across the solve only the sums and two
// flags are live (the registers are the solve's), and a lane only ever reads back what it stored itself.  A start that is not
// RUNNING, or whose factor failed, rides along on its own point and stores nothing (the failed factor: the rejection's lam,
// status and iters); a WAVE without a trial point skips the solve but not the staging, whose barriers are the workgroup's.
template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) fit_kernel(Consts K, FitArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  FitGroup<D> grp;
  grp.select_group(K, A.group_starts);
  const int64_t i = grp.start;
  const bool active = i < A.n;
  for (int it = 0; it < A.n_iter; ++it) {
    bool running = false, ok = false;
    double pq[3] = {1000.0, K.a_def, K.b_def}, inv_den;
    if (active) {
      double q[D], g[D], H[D * D], lam, qt[D];
      fit_load<D>(A, i, q, g, H, lam);
      running = A.status[i] == RSF_FIT_RUNNING;
      ok = running && fit_trial<D>(q, g, H, lam, A, qt);
      pq[0] = ok ? qt[0] : q[0];
      if constexpr (D == 3) { pq[1] = ok ? qt[1] : q[1]; pq[2] = ok ? qt[2] : q[2]; }
    }
    grp.perturb(A.fd, pq, inv_den);
    grp.template solve_group<DAMP>(lds, K, pq, inv_den, __any(ok) != 0);
    if (running) {
      double q[D], g[D], H[D * D], lam, qt[D], H_n[D * D], ssq = A.ssq[i];
      int32_t status = RSF_FIT_RUNNING, iters = A.iters[i];
      fit_load<D>(A, i, q, g, H, lam);
#pragma unroll
      for (int p = 0; p < D; ++p) qt[p] = q[p];
      if (ok) (void)fit_trial<D>(q, g, H, lam, A, qt);  // the point the group solved at, again
      grp.full(H_n);
      const int change = fit_decide<D>(q, ssq, g, H, lam, status, iters, ok, qt, grp.ssq, grp.xtr, H_n, A.ftol);
      fit_store<D>(A, i, change, q, ssq, g, H, lam, status, iters);
    }
  }
}

}  // namespace rsfk
