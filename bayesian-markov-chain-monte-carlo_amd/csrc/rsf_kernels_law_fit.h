// rsf_kernels_law_fit.h — the multi-start Levenberg-Marquardt fit around the state-law solve (include/rsf_law_fit.h): LawFitGroup,
// FitGroup's lane arrangement with the sample rule of an observable in it, law_fit_normal_kernel (the normal equations at a point)
// and law_fit_kernel, the fused hot path.  The halves of the iteration and a start's state (fit_trial, fit_decide, fit_load,
// fit_store, FitArgs) are rsf_kernels_fit.h's (only fit_kernel's loop is restated), the step rsf_kernels_law.h's law_step, the
// sample and its residual rsf_kernels_observe.h's observe_sample, the staging law_dr_solve's.  Included by rsf_law_fit.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_law_fit.h"
#include "rsf_kernels_fit.h"
#include "rsf_kernels_observe.h"

namespace rsfk {

// FitGroup's lanes, moves and sums with two things restated because they differ: the sample, which here is a value of the lane's own
// trajectory with a residual of its own (observe_sample's), and sample 0, which here depends on the lane's parameters
// (mu_0 = k' ms_0, theta_0 = x_0 Dc / V_ref) and so goes through the same exchange as every other sample.
template <int D>
struct LawFitGroup : FitGroup<D> {
  using Base = FitGroup<D>;
  __device__ __forceinline__ void reset() {
    this->ssq = 0.0;
#pragma unroll
    for (int p = 0; p < D; ++p) this->xtr[p] = 0.0;
#pragma unroll
    for (int e = 0; e < D * D; ++e) this->xtx[e] = 0.0;
  }
  // an output sample is complete (every lane of the group calls, in converged control flow): s this lane's sample, res its residual.
  // Lane 0's res is BROADCAST, not formed again from its sample: for the acceleration res is one fma of the velocity difference,
  // an ulp of the sample away from s - obs, and the sum of squares is rsf_law_observe's bit for bit.
  __device__ __forceinline__ void sample(double s, double res, double inv_den) {
    const double s0 = Base::template from_lane<0>(s);
    const double r = Base::template from_lane<0>(res);
    const double x = (s - s0) * inv_den;  // lane p + 1: the sensitivity to parameter p; lane 0: 0
    double xs[D];
    this->template gather<0>(x, xs);
    this->ssq = __builtin_fma(r, r, this->ssq);
#pragma unroll
    for (int p = 0; p < D; ++p) {
      this->xtr[p] = __builtin_fma(xs[p], r, this->xtr[p]);
#pragma unroll
      for (int r2 = p; r2 < D; ++r2) this->xtx[p * D + r2] = __builtin_fma(xs[p], xs[r2], this->xtx[p * D + r2]);
    }
  }
  // The group solve at the point pq (this lane's, perturbed) against the series of `observable` (RSF_OBS_*, a kernel argument:
  // wave-uniform, its branch taken once per output sample outside law_step).  Every thread of the workgroup calls: the staging's
  // barriers are the workgroup's, a wave with solve == false (wave-uniform) skips the steps and only the steps, a table that is
  // RESIDENT (K.nchunks == 1) is staged once per launch (`staged` remembers).  The arithmetic of a lane is law_observe_kernel's,
  // call for call.  No tier, no guard: a NaN trajectory runs to its end and gives sums that are not finite.
  template <int LAW, bool DAMP>
  __device__ __forceinline__ void solve_group(double *lds, const Consts &K, int32_t observable, const double (&pq)[3], double inv_den, bool solve, bool &staged) {
    const double *ld = lds + rsf::lds_data_offset(K);
    const rsf::Lane L = rsf::make_lane<DAMP>(pq[0], pq[1], pq[2], K);
    const rsf::State s0 = rsf::initial_state(pq[0], L, K);
    double ms = s0.ms, x = s0.x, V = s0.V, vprev = s0.V;
    // law_observe_kernel's per-lane factor and sample 0, restated as in law_dr_solve
    const double scale = observable == RSF_OBS_THETA ? pq[0] * K.inv_vref : L.kprime;
    const double first = observable == RSF_OBS_ACC ? 0.0 : observable == RSF_OBS_VELOCITY ? s0.V : observable == RSF_OBS_MU ? scale * s0.ms : s0.x * scale;
    int phase = 0;  // RK4 steps since the last output sample (wave-uniform)
    reset();
    for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
      const int kn = min(K.kc, K.nout - k0);
      if (K.nchunks > 1 || !staged) rsf::stage_chunk(lds, K, k0, kn);  // workgroup-uniform
      staged = true;
      if (!solve) continue;
      if (k0 == 1) sample(first, first - lds[rsf::lds_d0_offset(K)], inv_den);  // sample 0: (s_0 - data_0)^2 and its sensitivities
      const int nsteps = K.S * kn;
      int ko = 0;
      for (int r = 0; r < nsteps; ++r) {
        const double *v = lds + 2 * r;
        V = __builtin_fma(L.h6v, law_step<LAW, DAMP>(ms, x, v[0], v[1], v[2], L, K), V);
        if (++phase == K.S) {
          phase = 0;
          double s, res;
          observe_sample(observable, V, vprev, ms, x, scale, ld[ko], K, s, res);
          sample(s, res, inv_den);
          ++ko;
        }
      }
    }
  }
};

template <int D, int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) law_fit_normal_kernel(Consts K, FitArgs A, int32_t observable) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  LawFitGroup<D> grp;
  grp.select_group(K, A.group_starts);
  const int64_t i = grp.start;
  const bool active = i < A.n;
  double pq[3] = {1000.0, K.a_def, K.b_def}, inv_den;  // a lane without a start rides along on a harmless point
  if (active) {
    pq[0] = A.q[i * D];
    if constexpr (D == 3) { pq[1] = A.q[i * D + 1]; pq[2] = A.q[i * D + 2]; }
  }
  grp.perturb(A.fd, pq, inv_den);
  bool staged = false;
  grp.template solve_group<LAW, DAMP>(lds, K, observable, pq, inv_den, true, staged);
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

// The fused kernel's register budget: three workgroups per CU, i.e. three waves per SIMD and at most 168 registers, which is what 48 KB
// of LDS per workgroup admits at nsteps 2000.  Under kMinBlocks (two) seven of the eight instances take 129 to 152 registers anyway and
// the eighth (d = 1, slip, damped) 173 for the same loops, instruction for instruction; under this bound it takes 133 and the
// others what they took.  No instance has scratch.
constexpr int kLawFitBlocks = 3;

// The fused hot path: fit_kernel around LawFitGroup's solve.  fit_kernel's LOOP IS RESTATED here, statement for statement, and
// nothing else: as a template shared with fit_kernel it would change that kernel's instructions (rsf_kernels_law_dr.h has the
// trial of the same idea for dr_kernel), and the parent build's kernels stay as they are.  Per iteration every lane of a group
// reads its start's state, forms the same trial point, the group solves there, every lane reads the state again, takes the same
// decision from the same sums and stores the same values; across the solve only the sums and two flags are live.
template <int D, int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kLawFitBlocks) law_fit_kernel(Consts K, FitArgs A, int32_t observable) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  LawFitGroup<D> grp;
  grp.select_group(K, A.group_starts);
  const int64_t i = grp.start;
  const bool active = i < A.n;
  bool staged = false;
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
    grp.template solve_group<LAW, DAMP>(lds, K, observable, pq, inv_den, __any(ok) != 0, staged);
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
