// rsf_kernels_law_dr.h — the delayed-rejection sampler around the state-law solve (include/rsf_law_dr.h): law_dr_solve, dr_solve
// with the plain float64 RK4 under either law and the caller's observable in it, law_dr_ssq_kernel (one stage's solve alone) and
// law_dr_kernel, the fused hot path.  The pieces of the iteration are rsf_kernels_dr.h's (only dr_kernel's loop is restated), the
// step rsf_kernels_law.h's law_step, the sample and its residual rsf_kernels_observe.h's observe_sample.  Included by
// rsf_law_dr.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_law_dr.h"
#include "rsf_kernels_dr.h"
#include "rsf_kernels_observe.h"

namespace rsfk {

// SSq of the lane's point y where inb against the series of `observable` (RSF_OBS_*, a kernel argument: wave-uniform, its branch
// taken once per output sample outside law_step), in dr_solve's arrangement: a lane without a point rides along with the
// harmless point (1000, a_def, b_def), a WAVE without a point skips the steps — and only the steps: stage_chunk's barriers are
// taken by every wave of the workgroup whatever its lanes need.  A table that is RESIDENT (K.nchunks == 1) is staged once per
// launch (`staged` remembers).  The arithmetic is law_observe_kernel's, call for call: the SSq is rsf_law_observe's bit for bit,
// whatever the lane's neighbours are.  No tier, no guard: a NaN trajectory runs to its end and gives a non-finite SSq.
// STIFF (rsf_kernels_stiff.h): the spring's stiffness is `stiffness` (a kernel argument: wave-uniform), independent of Dc; the lane
// forms kappa = stiffness Dc and its IEEE reciprocal once per solve for make_lane and initial_state, and nothing else differs.
template <int D, int LAW, bool DAMP, bool STIFF = false>
__device__ __forceinline__ double law_dr_solve(double *lds, const Consts &K, int32_t observable, bool inb, const double (&y)[D], bool &staged,
                                               double stiffness = 0.0) {
  const double *ld = lds + rsf::lds_data_offset(K);
  double pq[3] = {1000.0, K.a_def, K.b_def};
  if (inb) {
    pq[0] = y[0];
    if constexpr (D == 3) { pq[1] = y[1]; pq[2] = y[2]; }
  }
  const bool solve = __any(inb) != 0;  // wave-uniform
  // D = 1: (a, b) are the model's for every lane and every stage, so the compiler would lift the lane constants made of them out of
  // the fused kernel's stage loop and hold them in vector registers across the whole iteration: 174 to 180 registers, past the
  // three-wave bracket of 168.  Opaque here, they are formed per stage as at D = 3: the same operations on the same values.
  if constexpr (D == 1) asm volatile("" : "+v"(pq[1]), "+v"(pq[2]));
  double kappa = 0.0, ikappa = 0.0;
  if constexpr (STIFF) {
    kappa = stiffness * pq[0];
    ikappa = 1.0 / kappa;
  }
  const rsf::Lane L = rsf::make_lane<DAMP, STIFF>(pq[0], pq[1], pq[2], K, kappa, ikappa);
  const rsf::State s0 = rsf::initial_state<STIFF>(pq[0], L, K, ikappa);
  double ms = s0.ms, x = s0.x, V = s0.V, vprev = s0.V, ssq = 0.0;
  // law_observe_kernel's per-lane factor and sample 0, RESTATED: as functions shared with that kernel they change its instructions
  // (the operands of one product swap), and the parent build's kernels stay as they are
  const double scale = observable == RSF_OBS_THETA ? pq[0] * K.inv_vref : L.kprime;
  const double first = observable == RSF_OBS_ACC ? 0.0 : observable == RSF_OBS_VELOCITY ? s0.V : observable == RSF_OBS_MU ? scale * s0.ms : s0.x * scale;
  int phase = 0;  // RK4 steps since the last output sample (wave-uniform)
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    if (K.nchunks > 1 || !staged) rsf::stage_chunk(lds, K, k0, kn);  // workgroup-uniform
    staged = true;
    if (k0 == 1) {
      const double r0 = first - lds[rsf::lds_d0_offset(K)];
      ssq = r0 * r0;  // (s_0 - data_0)^2
    }
    if (!solve) continue;
    const int nsteps = K.S * kn;
    int ko = 0;
    for (int r = 0; r < nsteps; ++r) {
      const double *v = lds + 2 * r;
      V = __builtin_fma(L.h6v, law_step<LAW, DAMP>(ms, x, v[0], v[1], v[2], L, K), V);
      if (++phase == K.S) {
        phase = 0;
        double s, res;
        observe_sample(observable, V, vprev, ms, x, scale, ld[ko], K, s, res);
        ssq = __builtin_fma(res, res, ssq);
        ++ko;
      }
    }
  }
  return ssq;
}

// one stage's SSq alone in the fused kernel's lane arrangement: ssq_out[i] where mask[i] != 0, nothing elsewhere
template <int D, int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks)
law_dr_ssq_kernel(Consts K, DrArgs A, int32_t observable, const double *__restrict__ y, const uint8_t *__restrict__ mask, double *__restrict__ ssq_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  dr_select_group(K, A, (int64_t)blockIdx.x * blockDim.x);
  const bool inb = i < A.n && mask[i] != 0;
  double x[D];
#pragma unroll
  for (int p = 0; p < D; ++p) x[p] = inb ? y[i * D + p] : 0.0;
  bool staged = false;
  const double ssq = law_dr_solve<D, LAW, DAMP>(lds, K, observable, inb, x, staged);
  if (inb) ssq_out[i] = ssq;
}

// The fused hot path: dr_kernel around law_dr_solve.  dr_kernel's LOOP IS RESTATED here, statement for statement, and nothing
// else: as a template over the solve that both kernels call it changes dr_kernel's instructions (tried: a forced-inline function
// taking the solve as a functor; tools/kernel_diff.py showed all four dr_kernel instances re-allocated), and the parent build's
// kernels stay as they are.  Every piece of the iteration — dr_stage1, dr_stage2, dr_decide2, dr_log_uniforms, dr_logtarget,
// dr_healthy, dr_factor, dr_select_group, DrArgs — is rsf_kernels_dr.h's own.
template <int D, int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) law_dr_kernel(Consts K, DrArgs A, int32_t observable) {
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
    const double ssq = law_dr_solve<D, LAW, DAMP>(lds, K, observable, inb, xn, staged);
    // the chain's index, opaque after the solve: the addresses of its counters and trace rows are formed here, stage by stage,
    // instead of being held in registers across the solve (they are invariant in this loop, and the compiler lifts them out of it)
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
