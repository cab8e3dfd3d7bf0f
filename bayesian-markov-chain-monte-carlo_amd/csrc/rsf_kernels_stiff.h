// rsf_kernels_stiff.h — the state-law solve and its delayed-rejection sampler with the spring's stiffness a constant of the
// apparatus, independent of Dc (include/rsf_stiff.h): stiff_observe_kernel, stiff_dr_ssq_kernel and stiff_dr_kernel, the fused hot
// path.  The lane forms kappa = stiffness Dc and ikappa = 1.0 / kappa, one IEEE division per lane per solve, and rsf_device.h's
// make_lane<DAMP, true> / initial_state<true> read them where the reference's coupling k' = 1e-2 * 10 / Dc has its literal and
// that literal's reciprocal:
//     kprime = kappa inv_dc      beta = (b V_ref) ikappa      ms_0 = (mu_0 Dc) ikappa
// Every other lane constant, law_rhs, law_step and observe_sample are called as they are; theta's factor Dc (1 / V_ref) is
// unchanged and the friction's factor is the new kprime.  On a lane where stiffness Dc == 0.1 exactly, every constant is the
// coupled kernel's bit for bit.  `stiffness` is a kernel argument: wave-uniform, so it lives in scalar registers.  No guard
// against a stiffness below the critical (b - a) / Dc: the trajectory runs to its end and gives a non-finite SSq.
//
// The solve of the two sampler kernels is rsf_kernels_law_dr.h's law_dr_solve<D, LAW, DAMP, true>, shared.  The kernels' own
// statements — law_observe_kernel's, law_dr_ssq_kernel's, law_dr_kernel's loop — are RESTATED: as device functions that the
// coupled kernels call too they change those kernels' instructions (tried: forced-inline bodies templated on STIFF;
// tools/kernel_diff.py showed every law_observe_kernel, law_dr_ssq_kernel and law_dr_kernel instance changed), and the parent
// build's kernels stay as they are.  Included by rsf_stiff.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_stiff.h"
#include "rsf_kernels_law_dr.h"

namespace rsfk {

// law_observe_kernel (rsf_kernels_observe.h), statement for statement, with the lane made from (kappa, ikappa)
template <int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock)
stiff_observe_kernel(Consts K, int32_t observable, double stiffness, int64_t n, const double *__restrict__ dc, const double *__restrict__ a,
                     const double *__restrict__ b, double *__restrict__ ssq_out, double *__restrict__ series_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  const bool want_ssq = ssq_out != nullptr, want_series = series_out != nullptr;
  const double dci = active ? dc[i] : 1000.0;
  const double kappa = stiffness * dci, ikappa = 1.0 / kappa;
  const rsf::Lane L = rsf::make_lane<DAMP, true>(dci, (active && a) ? a[i] : K.a_def, (active && b) ? b[i] : K.b_def, K, kappa, ikappa);
  const rsf::State s0 = rsf::initial_state<true>(dci, L, K, ikappa);
  double ms = s0.ms, x = s0.x, V = s0.V, vprev = s0.V, ssq = 0.0;
  const double scale = observable == RSF_OBS_THETA ? dci * K.inv_vref : L.kprime;
  const double first = observable == RSF_OBS_ACC ? 0.0
                       : observable == RSF_OBS_VELOCITY ? s0.V
                       : observable == RSF_OBS_MU ? scale * s0.ms : s0.x * scale;
  double *series_i = want_series ? series_out + i : nullptr;
  const bool store = want_series && active;
  if (store) series_i[0] = first;
  const bool work = rsf::ballot(active) != 0;            // wave-uniform
  const double *ld = lds + rsf::lds_data_offset(K);
  int phase = 0;                                         // RK4 steps since the last output sample (wave-uniform)
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    rsf::stage_chunk(lds, K, k0, kn);
    if (want_ssq && k0 == 1) {
      const double r0 = first - lds[rsf::lds_d0_offset(K)];
      ssq = r0 * r0;                                     // (s_0 - data_0)^2
    }
    if (!work) continue;
    const int nsteps = K.S * kn;
    int ko = 0;
    for (int r = 0; r < nsteps; ++r) {
      const double *v = lds + 2 * r;
      V = __builtin_fma(L.h6v, law_step<LAW, DAMP>(ms, x, v[0], v[1], v[2], L, K), V);
      if (++phase == K.S) {
        phase = 0;
        const double obs = want_ssq ? ld[ko] : 0.0;
        double s, res;                                   // the sample and its residual
        observe_sample(observable, V, vprev, ms, x, scale, obs, K, s, res);
        if (store) series_i[(int64_t)(k0 + ko) * n] = s;
        if (want_ssq) ssq = __builtin_fma(res, res, ssq);
        ++ko;
      }
    }
  }
  if (want_ssq && active) ssq_out[i] = ssq;
}

// law_dr_ssq_kernel with the stiffness: one stage's SSq alone in the fused kernel's lane arrangement
template <int D, int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks)
stiff_dr_ssq_kernel(Consts K, DrArgs A, int32_t observable, double stiffness, const double *__restrict__ y, const uint8_t *__restrict__ mask,
                    double *__restrict__ ssq_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  dr_select_group(K, A, (int64_t)blockIdx.x * blockDim.x);
  const bool inb = i < A.n && mask[i] != 0;
  double x[D];
#pragma unroll
  for (int p = 0; p < D; ++p) x[p] = inb ? y[i * D + p] : 0.0;
  bool staged = false;
  const double ssq = law_dr_solve<D, LAW, DAMP, true>(lds, K, observable, inb, x, staged, stiffness);
  if (inb) ssq_out[i] = ssq;
}

// The fused hot path: law_dr_kernel's loop (dr_kernel's, rsf_kernels_dr.h), statement for statement, around the solve with the
// stiffness: n_iter iterations per launch, one lane per chain, a wave with no point in the box skips the steps, a resident table
// is staged once per launch.  Every piece of the iteration is rsf_kernels_dr.h's own.
template <int D, int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) stiff_dr_kernel(Consts K, DrArgs A, int32_t observable, double stiffness) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < A.n;
  const uint64_t gid = (uint64_t)(A.offset + i);
  dr_select_group(K, A, (int64_t)blockIdx.x * blockDim.x);
  const double *L = dr_factor<D>(A, (int64_t)blockIdx.x * blockDim.x);  // workgroup-uniform
  double x[D], lx = active ? A.l[i] : 0.0;
#pragma unroll
  for (int p = 0; p < D; ++p) x[p] = active ? A.q[i * D + p] : 0.5 * (A.lo[p] + A.hi[p]);
  double l1 = -INFINITY;
  bool pend = false, staged = false;
  const int step = A.stages == 2 ? 1 : 2;
  for (int ss = 0; ss < 2 * A.n_iter; ss += step) {
    const uint32_t it = A.iter + (uint32_t)(ss >> 1);
    const bool second = (ss & 1) != 0;  // launch-uniform
    const bool want = second ? pend : (active && dr_healthy<D>(A, x, lx));
    double xn[D];
    bool inb = false;
    if (want) inb = second ? dr_stage2<D>(A, L, gid, it, x, xn) : dr_stage1<D>(A, L, gid, it, x, xn);
    const double ssq = law_dr_solve<D, LAW, DAMP, true>(lds, K, observable, inb, xn, staged, stiffness);
    // the chain's index, opaque after the solve (law_dr_kernel's note)
    int64_t j = i;
    asm volatile("" : "+v"(j));
    const double ln = inb ? dr_logtarget(ssq, A.shape) : -INFINITY;
    double log_u1, log_u2;
    dr_log_uniforms(A, gid, it, log_u1, log_u2);
    bool acc;
    if (!second) {
      acc = inb && accept_test(ln - lx, log_u1);
      l1 = ln;
      pend = want && !acc && A.stages == 2;
      if (active) {
        if (acc) A.accepted1[j] += 1;
        else if (!want) A.stuck[j] += 1;
        else if (!inb) A.outbox1[j] += 1;
      }
    } else {
      acc = inb && dr_decide2<D>(A, gid, it, lx, l1, ln, log_u2);
      if (acc) A.accepted2[j] += 1;
      else if (want && !inb) A.outbox2[j] += 1;
    }
    if (acc) {
#pragma unroll
      for (int p = 0; p < D; ++p) x[p] = xn[p];
      lx = ln;
    }
    if (A.tq && active && (second || A.stages == 1)) {  // the state after the iteration
      const int64_t row = (int64_t)(ss >> 1) * A.n + j;
#pragma unroll
      for (int p = 0; p < D; ++p) A.tq[row * D + p] = x[p];
      A.tl[row] = lx;
    }
  }
  if (active) {
#pragma unroll
    for (int p = 0; p < D; ++p) A.q[i * D + p] = x[p];
    A.l[i] = lx;
  }
}

}  // namespace rsfk
