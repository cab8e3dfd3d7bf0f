// rsf_kernels_kstiff.h — the delayed-rejection sampler of the state-law solve with the spring's stiffness AMONG THE PARAMETERS
// (include/rsf_kstiff.h): chains over (Dc, k) at D = 2 or (Dc, a, b, k) at D = 4, the stiffness the last coordinate.
// kstiff_observe_kernel (stiff_observe_kernel with k read per lane), kstiff_dr_ssq_kernel, kstiff_dr_kernel (the fused hot path)
// and the split pair kstiff_dr_propose_kernel / kstiff_dr_accept_kernel.
//
// The solve is rsf_kernels_law_dr.h's law_dr_solve<D - 1, LAW, DAMP, true>, shared: it takes the stiffness by value, here the lane's
// own — a vector register in place of rsf_kernels_stiff.h's scalar, and nothing else differs: kappa = k Dc and the IEEE division
// 1.0 / kappa once per lane per solve.  A lane without a point rides along with (1000, a_def, b_def) and k = 1e-4 (kappa = 0.1, the
// coupling's value).  The chain logic is rsf_kernels_dr.h's, which takes the argument block as a deduced parameter: KDrArgs below is
// DrArgs' members with lo / hi of four parameters (DrArgs is a kernel argument of every parent instance and stays as it is).
// The kernels' own statements — stiff_observe_kernel's, stiff_dr_ssq_kernel's, stiff_dr_kernel's loop, dr_propose_kernel's and
// dr_accept_kernel's bodies — are RESTATED, as rsf_kernels_stiff.h restates law_dr_kernel's: a kernel templated on its argument
// block has another name, and the parent build's kernels keep theirs.  Included by rsf_kstiff.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_kstiff.h"
#include "rsf_kernels_law_dr.h"

namespace rsfk {

struct KDrArgs {
  int64_t n, offset;
  int64_t group_chains;  // chains per group (observation series and factor); 0: one group for all
  uint64_t seed;
  uint32_t iter;         // Philox iteration of the call's first iteration
  int32_t n_iter;
  int32_t stages;        // the fused kernel: 1 or 2 stages per iteration; the split kernels: the stage of the call, 1 or 2
  double gamma, shape;
  double lo[RSF_KSTIFF_MAX_PARAMS], hi[RSF_KSTIFF_MAX_PARAMS];
  const double *chol;    // [groups][D (D + 1) / 2], row-major lower triangles: one small device array
  double *q, *l;         // [n][d], [n]
  int32_t *accepted1, *accepted2, *outbox1, *outbox2, *stuck;  // [n] each
  double *tq, *tl;       // traces, iteration-major: tq[n_iter][n][d], tl[n_iter][n]; both NULL or both set
};

constexpr double kKstiffIdle = 1e-4;  // the stiffness of a lane without a point: kappa = 1e-4 * 1000 = 0.1

// SSq of the lane's point y = (Dc[, a, b], k) where inb: law_dr_solve on the first D - 1 coordinates with the lane's own stiffness
template <int D, int LAW, bool DAMP>
__device__ __forceinline__ double kstiff_solve(double *lds, const Consts &K, int32_t observable, bool inb, const double (&y)[D], bool &staged) {
  double p[D - 1];
#pragma unroll
  for (int c = 0; c < D - 1; ++c) p[c] = y[c];
  return law_dr_solve<D - 1, LAW, DAMP, true>(lds, K, observable, inb, p, staged, inb ? y[D - 1] : kKstiffIdle);
}

// stiff_observe_kernel (rsf_kernels_stiff.h), statement for statement, with the stiffness k[i] of the lane
template <int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock)
kstiff_observe_kernel(Consts K, int32_t observable, int64_t n, const double *__restrict__ dc, const double *__restrict__ a, const double *__restrict__ b,
                      const double *__restrict__ k, double *__restrict__ ssq_out, double *__restrict__ series_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  const bool want_ssq = ssq_out != nullptr, want_series = series_out != nullptr;
  const double dci = active ? dc[i] : 1000.0;
  const double kappa = (active ? k[i] : kKstiffIdle) * dci, ikappa = 1.0 / kappa;
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

// stiff_dr_ssq_kernel with the stiffness the point's last coordinate: one stage's SSq alone in the fused kernel's lane arrangement
template <int D, int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks)
kstiff_dr_ssq_kernel(Consts K, KDrArgs A, int32_t observable, const double *__restrict__ y, const uint8_t *__restrict__ mask, double *__restrict__ ssq_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  dr_select_group(K, A, (int64_t)blockIdx.x * blockDim.x);
  const bool inb = i < A.n && mask[i] != 0;
  double x[D];
#pragma unroll
  for (int p = 0; p < D; ++p) x[p] = inb ? y[i * D + p] : 0.0;
  bool staged = false;
  const double ssq = kstiff_solve<D, LAW, DAMP>(lds, K, observable, inb, x, staged);
  if (inb) ssq_out[i] = ssq;
}

// The fused hot path: stiff_dr_kernel's loop (law_dr_kernel's, dr_kernel's), statement for statement, around the solve with the
// lane's stiffness: n_iter iterations per launch, one lane per chain, a wave with no point in the box skips the steps, a resident
// table is staged once per launch.  Every piece of the iteration is rsf_kernels_dr.h's own.
template <int D, int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) kstiff_dr_kernel(Consts K, KDrArgs A, int32_t observable) {
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
    const double ssq = kstiff_solve<D, LAW, DAMP>(lds, K, observable, inb, xn, staged);
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

// ---- the split kernels: dr_propose_kernel's and dr_accept_kernel's bodies (rsf_kernels_dr.h), statement for statement ---------------
template <int D>
__global__ void __launch_bounds__(kMaxBlock) kstiff_dr_propose_kernel(KDrArgs A, const uint8_t *__restrict__ pending, double *__restrict__ y,
                                                                      uint8_t *__restrict__ mask) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.n) return;
  double x[D], xn[D];
#pragma unroll
  for (int p = 0; p < D; ++p) x[p] = A.q[j * D + p];
  const double *L = dr_factor<D>(A, j);
  const uint64_t gid = (uint64_t)(A.offset + j);
  bool inb = false;
  const bool want = A.stages == 1 ? dr_healthy<D>(A, x, A.l[j]) : pending[j] != 0;
  if (want) inb = A.stages == 1 ? dr_stage1<D>(A, L, gid, A.iter, x, xn) : dr_stage2<D>(A, L, gid, A.iter, x, xn);
#pragma unroll
  for (int p = 0; p < D; ++p) y[j * D + p] = want ? xn[p] : x[p];
  mask[j] = inb ? 1 : 0;
}

template <int D>
__global__ void __launch_bounds__(kMaxBlock)
kstiff_dr_accept_kernel(KDrArgs A, const double *__restrict__ y, const uint8_t *__restrict__ mask, const double *__restrict__ ssq, double *__restrict__ l1,
                        uint8_t *__restrict__ pending) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.n) return;
  const uint64_t gid = (uint64_t)(A.offset + j);
  const double lx = A.l[j];
  const bool inb = mask[j] != 0;
  const double ln = inb ? dr_logtarget(ssq[j], A.shape) : -INFINITY;
  double log_u1, log_u2;
  dr_log_uniforms(A, gid, A.iter, log_u1, log_u2);
  bool acc = false;
  if (A.stages == 1) {
    double x[D];
#pragma unroll
    for (int p = 0; p < D; ++p) x[p] = A.q[j * D + p];
    const bool want = dr_healthy<D>(A, x, lx);
    acc = inb && accept_test(ln - lx, log_u1);
    l1[j] = ln;
    pending[j] = (want && !acc) ? 1 : 0;
    if (acc) A.accepted1[j] += 1;
    else if (!want) A.stuck[j] += 1;
    else if (!inb) A.outbox1[j] += 1;
  } else {
    const bool want = pending[j] != 0;
    acc = inb && dr_decide2<D>(A, gid, A.iter, lx, l1[j], ln, log_u2);
    if (acc) A.accepted2[j] += 1;
    else if (want && !inb) A.outbox2[j] += 1;
  }
  if (acc) {
#pragma unroll
    for (int p = 0; p < D; ++p) A.q[j * D + p] = y[j * D + p];
    A.l[j] = ln;
  }
}

}  // namespace rsfk
