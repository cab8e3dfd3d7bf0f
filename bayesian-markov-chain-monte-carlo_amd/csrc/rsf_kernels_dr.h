// rsf_kernels_dr.h — two-stage delayed-rejection Metropolis over the strict box (include/rsf_dr.h; tests/dr_reference.py is the
// specification): dr_stage1 / dr_stage2 / dr_decide2, the iteration's pieces as device functions defined ONCE, the split kernels
// dr_propose_kernel / dr_accept_kernel around them, dr_ssq_kernel (one stage's solve alone) and dr_kernel, the fused hot path in
// smc_move_kernel's arrangement.  Included by rsf_dr.hip and, for the chain logic around the state-law solve, by rsf_kernels_law_dr.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_dr.h"
#include "rsf_kernel_common.h"
#include "rsf_device.h"

namespace rsfk {

constexpr uint32_t kDrSlotZ01 = 5, kDrSlotZ2 = 6;  // Philox slots of the second stage's normals (0..2: rsf_device.h; 3, 4: ensemble partner, SMC resampling)

struct DrArgs {
  int64_t n, offset;
  int64_t group_chains;  // chains per group (observation series and factor); 0: one group for all
  uint64_t seed;
  uint32_t iter;         // Philox iteration of the call's first iteration
  int32_t n_iter;
  int32_t stages;        // the fused kernel: 1 or 2 stages per iteration; the split kernels: the stage of the call, 1 or 2
  double gamma, shape;
  double lo[RSF_DR_MAX_PARAMS], hi[RSF_DR_MAX_PARAMS];
  const double *chol;    // [groups][D (D + 1) / 2], row-major lower triangles: one small device array
  double *q, *l;         // [n][d], [n]
  int32_t *accepted1, *accepted2, *outbox1, *outbox2, *stuck;  // [n] each
  double *tq, *tl;       // traces, iteration-major: tq[n_iter][n][d], tl[n_iter][n]; both NULL or both set
};

// l = -shape log SSq; -inf where SSq is not finite or not positive: smc_logtarget's expression (rsf_kernels_smc.h belongs to rsf_smc.hip)
__device__ __forceinline__ double dr_logtarget(double ssq, double shape) {
  return (__builtin_isfinite(ssq) && ssq > 0.0) ? -shape * log(ssq) : -INFINITY;
}

// The pieces below take the argument block as a deduced parameter ARGS: DrArgs here, and rsf_kernels_kstiff.h's wider block
// (lo / hi of four parameters) — DrArgs itself is a kernel argument of every instance of this family and stays as it is.

// a chain that may move: strictly inside the box with a finite l
template <int D, class ARGS>
__device__ __forceinline__ bool dr_healthy(const ARGS &A, const double (&x)[D], double l) {
  return in_box<D>(x, A) && __builtin_isfinite(l);
}

// the D normals of (seed, gid, it) from the slots s01 (components 0 and 1) and s2 (component 2): smc_proposal's draws for slots 0 and 1
template <int D, class ARGS>
__device__ __forceinline__ void dr_normals(const ARGS &A, uint64_t gid, uint32_t it, uint32_t s01, uint32_t s2, double (&z)[4]) {
  uint32_t w[4];
  z[0] = z[1] = z[2] = z[3] = 0.0;
  rsf::draw_words(A.seed, gid, it, s01, w);
  rsf::normal_pair(w, z[0], z[1]);
  if (D > 2) { rsf::draw_words(A.seed, gid, it, s2, w); rsf::normal_pair(w, z[2], z[3]); }
}

// the logarithms of the two accept uniforms of (seed, gid, it): U1 = u53(w0, w1), U2 = u53(w2, w3) of the accept slot
template <class ARGS>
__device__ __forceinline__ void dr_log_uniforms(const ARGS &A, uint64_t gid, uint32_t it, double &log_u1, double &log_u2) {
  uint32_t w[4];
  rsf::draw_words(A.seed, gid, it, rsf::SLOT_U, w);
  log_u1 = rsf::rng_log(rsf::u53(w[0], w[1]));
  log_u2 = rsf::rng_log(rsf::u53(w[2], w[3]));
}

// Stage 1: y1 = q + L z1 in propose<D>'s own arithmetic (smc_proposal's point) → inside the strict box?  L: the group's factor
template <int D, class ARGS>
__device__ __forceinline__ bool dr_stage1(const ARGS &A, const double *__restrict__ L, uint64_t gid, uint32_t it, const double (&q)[D],
                                          double (&y)[D]) {
  double z[4];
  dr_normals<D>(A, gid, it, rsf::SLOT_Z01, rsf::SLOT_Z2, z);
  propose<D>(q, [&](int k) { return L[k]; }, z, y);
  return in_box<D>(y, A);
}

// Stage 2: y2 = q + gamma (L z2), every product and sum rounded, in the specification's order → inside the strict box?
template <int D, class ARGS>
__device__ __forceinline__ bool dr_stage2(const ARGS &A, const double *__restrict__ L, uint64_t gid, uint32_t it, const double (&q)[D],
                                          double (&y)[D]) {
#pragma clang fp contract(off)
  double z[4];
  dr_normals<D>(A, gid, it, kDrSlotZ01, kDrSlotZ2, z);
  int e = 0;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    double v = L[e++] * z[0];
#pragma unroll
    for (int r = 1; r <= p; ++r) v = v + L[e++] * z[r];
    y[p] = q[p] + A.gamma * v;
  }
  return in_box<D>(y, A);
}

// The stage 2 decision for a proposal INSIDE the box, after a stage 1 that was rejected with l1 (-inf: outside the box or no
// target value there): log alpha2 = (l2 - l) + log q + log(1 - alpha1(y2, y1)) - log(1 - alpha1(q, y1)) against log U2.  Both
// stages' normals come from the stream again: nothing of them is kept across a solve.
template <int D, class ARGS>
__device__ __forceinline__ bool dr_decide2(const ARGS &A, uint64_t gid, uint32_t it, double l, double l1, double l2, double log_u2) {
#pragma clang fp contract(off)
  if (!__builtin_isfinite(l2)) return false;
  double z1[4], z2[4];
  dr_normals<D>(A, gid, it, rsf::SLOT_Z01, rsf::SLOT_Z2, z1);
  dr_normals<D>(A, gid, it, kDrSlotZ01, kDrSlotZ2, z2);
  double sw = 0.0, s1 = 0.0;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    const double w = z1[p] - A.gamma * z2[p];
    sw = sw + w * w;
    s1 = s1 + z1[p] * z1[p];
  }
  double la = (l2 - l) + -0.5 * (sw - s1);
  if (l1 != -INFINITY) {
    if (l1 >= l2) return false;
    la = (la + log(-expm1(l1 - l2))) - log(-expm1(l1 - l));
  }
  return accept_test(la, log_u2);
}

// the factor of chain j's group
template <int D, class ARGS>
__device__ __forceinline__ const double *dr_factor(const ARGS &A, int64_t j) {
  return A.chol + (A.group_chains > 0 ? j / A.group_chains : 0) * (D * (D + 1) / 2);
}

// ---- the split kernels: one thread per chain ---------------------------------------------------------------------------------------
// A.stages is the stage of the call.  Stage 1: every healthy chain proposes; stage 2: the chains whose pending byte is 1.
template <int D>
__global__ void __launch_bounds__(kMaxBlock) dr_propose_kernel(DrArgs A, const uint8_t *__restrict__ pending, double *__restrict__ y,
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
dr_accept_kernel(DrArgs A, const double *__restrict__ y, const uint8_t *__restrict__ mask, const double *__restrict__ ssq, double *__restrict__ l1,
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

// ---- one stage's solve, lane = chain: what dr_ssq_kernel and dr_kernel share --------------------------------------------------------
// SSq of the lane's point y where inb, in smc_move_kernel's arrangement: a lane without a point rides along with the harmless point
// (1000, a_def, b_def), a WAVE without a point skips the solve.  The table and the observation are staged chunk by chunk
// (rsf::stage_chunk, whose barriers every wave takes); a table that is RESIDENT (K.nchunks == 1) is staged once per launch — the
// first call stages it, `staged` remembers — because nothing writes it afterwards.
template <int D, bool DAMP>
__device__ __forceinline__ double dr_solve(double *lds, const Consts &K, bool inb, const double (&y)[D], bool &staged) {
  const double *ld = lds + rsf::lds_data_offset(K);
  double pq[3] = {1000.0, K.a_def, K.b_def};
  if (inb) {
    pq[0] = y[0];
    if constexpr (D == 3) { pq[1] = y[1]; pq[2] = y[2]; }
  }
  const bool solve = __any(inb) != 0;  // wave-uniform
  const rsf::Lane L = rsf::make_lane<DAMP>(pq[0], pq[1], pq[2], K);
  rsf::State st = rsf::initial_state(pq[0], L, K);
  double ssq = 0.0;
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    if (K.nchunks > 1 || !staged) rsf::stage_chunk(lds, K, k0, kn);  // workgroup-uniform
    staged = true;
    if (k0 == 1) {  // sample 0 belongs to no chunk: acc[0] = 0, so the observation's square starts the sum
      const double d0 = lds[rsf::lds_d0_offset(K)];
      ssq = d0 * d0;
    }
    if (solve)
      rsf::integrate_lockstep<DAMP>(lds, K, L, st, kn, [&](double ak, int ko) { const double r = ak - ld[ko]; ssq = __builtin_fma(r, r, ssq); }, [] {});
  }
  return ssq;
}

// the observation series of the workgroup whose first chain is `first` (a group's chains are whole workgroups)
template <class ARGS>
__device__ __forceinline__ void dr_select_group(Consts &K, const ARGS &A, int64_t first) {
  if (A.group_chains > 0) K.data += (first / A.group_chains) * K.nout;
}

template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) dr_ssq_kernel(Consts K, DrArgs A, const double *__restrict__ y, const uint8_t *__restrict__ mask,
                                                                      double *__restrict__ ssq_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  dr_select_group(K, A, (int64_t)blockIdx.x * blockDim.x);
  const bool inb = i < A.n && mask[i] != 0;
  double x[D];
#pragma unroll
  for (int p = 0; p < D; ++p) x[p] = inb ? y[i * D + p] : 0.0;
  bool staged = false;
  const double ssq = dr_solve<D, DAMP>(lds, K, inb, x, staged);
  if (inb) ssq_out[i] = ssq;
}

// ---- the fused hot path -------------------------------------------------------------------------------------------------------------
// One lane per chain, A.n_iter iterations inside the launch, the chain's state in registers as smc_move_kernel holds it.  ONE loop
// over the stages (two per iteration; with A.stages = 1 the second is stepped over), so the solve is compiled once.  Stage 1: every
// healthy chain proposes y1; stage 2: the lanes rejected at stage 1 propose y2.  Across a solve a lane keeps its state, its
// proposal, l1 and two flags; the normals and the uniforms of the decision are drawn again after the solve.
template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) dr_kernel(Consts K, DrArgs A) {
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
    const double ssq = dr_solve<D, DAMP>(lds, K, inb, xn, staged);
    const double ln = inb ? dr_logtarget(ssq, A.shape) : -INFINITY;
    double log_u1, log_u2;
    dr_log_uniforms(A, gid, it, log_u1, log_u2);
    bool acc;
    if (!second) {
      acc = inb && accept_test(ln - lx, log_u1);
      l1 = ln;
      pend = want && !acc && A.stages == 2;
      if (active) {
        if (acc) A.accepted1[i] += 1;
        else if (!want) A.stuck[i] += 1;
        else if (!inb) A.outbox1[i] += 1;
      }
    } else {
      acc = inb && dr_decide2<D>(A, gid, it, lx, l1, ln, log_u2);
      if (acc) A.accepted2[i] += 1;
      else if (want && !inb) A.outbox2[i] += 1;
    }
    if (acc) {
#pragma unroll
      for (int p = 0; p < D; ++p) x[p] = xn[p];
      lx = ln;
    }
    if (A.tq && active && (second || A.stages == 1)) {  // the state after the iteration
      const int64_t row = (int64_t)(ss >> 1) * A.n + i;
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
