// rsf_kernels_ensemble.h — the affine-invariant stretch move in island ensembles (include/rsf_ensemble.h; tests/ensemble_reference.py
// is the specification): ens_draws / ens_proposal / ens_decide, the half-step's pieces as device functions defined ONCE, the split
// kernels ensemble_propose_kernel / ensemble_accept_kernel around them, ensemble_ssq_kernel (a half-step's solve alone) and
// ensemble_move_kernel, the fused hot path in smc_move_kernel's arrangement.  Included by rsf_ensemble.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_ensemble.h"
#include "rsf_kernel_common.h"
#include "rsf_device.h"

namespace rsfk {

constexpr uint32_t kEnsSlotPartner = 3;  // Philox slot of the partner index: rsf_smc_init's third uniform's (0..2: rsf_device.h)

struct EnsArgs {
  int64_t n, offset;
  int64_t group_walkers;  // walkers per observation series (0: one series for all)
  uint64_t seed;
  uint32_t iter;          // Philox iteration of the call's first iteration
  int32_t n_iter;
  int32_t B;              // walkers per half island: the ctx's workgroup size
  int32_t half;           // the split kernels' moving half
  uint32_t logmask;
  double a, shape;
  double lo[RSF_ENSEMBLE_MAX_PARAMS], hi[RSF_ENSEMBLE_MAX_PARAMS];
  double *q, *l;                        // [n][d], [n]
  int32_t *accepted, *outbox, *stuck;   // [n] each
  double *tq, *tl;                      // traces, iteration-major: tq[n_iter][n][d], tl[n_iter][n]; both NULL or both set
};

// what became of a walker's half-step before the decision
enum EnsProposal : int { ENS_STUCK = 0, ENS_OUTSIDE = 1, ENS_INSIDE = 2 };

// l = -shape log SSq; -inf where SSq is not finite or not positive: smc_logtarget's expression (rsf_kernels_smc.h belongs to rsf_smc.hip)
__device__ __forceinline__ double ens_logtarget(double ssq, double shape) {
  return (__builtin_isfinite(ssq) && ssq > 0.0) ? -shape * log(ssq) : -INFINITY;
}

// a walker that may move: strictly inside the box with a finite l
template <int D>
__device__ __forceinline__ bool ens_healthy(const EnsArgs &A, const double (&x)[D], double l) {
  return in_box<D>(x, A) && __builtin_isfinite(l);
}

// the draws of (seed, particle gid, iteration it): the stretch uniform, the logarithm of the accept uniform, the partner index
__device__ __forceinline__ void ens_draws(const EnsArgs &A, uint64_t gid, uint32_t it, double &us, double &log_ua, int &r) {
  uint32_t w[4];
  rsf::draw_words(A.seed, gid, it, rsf::SLOT_U, w);
  log_ua = rsf::rng_log(rsf::u53(w[0], w[1]));
  us = rsf::u53(w[2], w[3]);
  rsf::draw_words(A.seed, gid, it, kEnsSlotPartner, w);
  r = (int)(((uint64_t)w[0] * (uint64_t)(uint32_t)A.B) >> 32);
}

// Steps 3 and 4 for a healthy walker x and its partner y: q' and J = (d - 1) log z + sum over masked p of (u'_p - u_p) → inside the
// strict box?  Compiled WITHOUT contraction: s and z are the IEEE operations the specification's NumPy takes, in its order, and
// the one fused multiply-add of the rule is written out.
template <int D>
__device__ __forceinline__ bool ens_proposal(const EnsArgs &A, double us, const double (&x)[D], const double (&y)[D], double (&qn)[D], double &J) {
#pragma clang fp contract(off)
  const double s = (A.a - 1.0) * us + 1.0;
  const double z = (s * s) / A.a;
  J = (double)(D - 1) * log(z);
#pragma unroll
  for (int p = 0; p < D; ++p) {
    const bool m = (A.logmask >> p) & 1u;  // wave-uniform
    const double u = m ? log(x[p]) : x[p], v = m ? log(y[p]) : y[p];
    const double un = __builtin_fma(z, u - v, v);
    qn[p] = m ? exp(un) : un;
    if (m) J += un - u;
  }
  return in_box<D>(qn, A);
}

// Step 5 for a proposal INSIDE the box: log alpha = J + (l' - l) against log U_a; a non-finite l' is rejected
__device__ __forceinline__ bool ens_decide(double J, double l, double ln, double log_ua) {
#pragma clang fp contract(off)
  return __builtin_isfinite(ln) && accept_test(J + (ln - l), log_ua);
}

// what the owning lane writes after the decision: the counter that grows, if any
__device__ __forceinline__ void ens_count(const EnsArgs &A, int64_t j, int found, bool acc) {
  if (acc) A.accepted[j] += 1;
  else if (found == ENS_OUTSIDE) A.outbox[j] += 1;
  else if (found == ENS_STUCK) A.stuck[j] += 1;
}

// the mover of thread t of a split launch (one thread per walker of the moving half) and the first walker of the other half of its island
__device__ __forceinline__ int64_t ens_mover(const EnsArgs &A, int64_t t, int64_t &other) {
  const int64_t base = (t / A.B) * (2 * (int64_t)A.B);
  other = base + (int64_t)(1 - A.half) * A.B;
  return base + (int64_t)A.half * A.B + t % A.B;
}

// ---- the split kernels: one thread per walker of the moving half; the partner is read from global q ---------------------------------
template <int D>
__global__ void __launch_bounds__(kMaxBlock) ensemble_propose_kernel(EnsArgs A, double *__restrict__ q_new, uint8_t *__restrict__ inbox,
                                                                     double *__restrict__ logz_jac) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= A.n / 2) return;
  int64_t other;
  const int64_t j = ens_mover(A, t, other);
  double x[D], y[D], qn[D], us, log_ua, J = 0.0;
  int r;
#pragma unroll
  for (int p = 0; p < D; ++p) x[p] = A.q[j * D + p];
  ens_draws(A, (uint64_t)(A.offset + j), A.iter, us, log_ua, r);
  bool inb = false;
  if (ens_healthy<D>(A, x, A.l[j])) {
#pragma unroll
    for (int p = 0; p < D; ++p) y[p] = A.q[(other + r) * D + p];
    inb = ens_proposal<D>(A, us, x, y, qn, J);
  } else {
#pragma unroll
    for (int p = 0; p < D; ++p) qn[p] = x[p];
  }
#pragma unroll
  for (int p = 0; p < D; ++p) q_new[j * D + p] = qn[p];
  inbox[j] = inb ? 1 : 0;
  logz_jac[j] = J;
}

template <int D>
__global__ void __launch_bounds__(kMaxBlock)
ensemble_accept_kernel(EnsArgs A, const double *__restrict__ q_new, const uint8_t *__restrict__ inbox, const double *__restrict__ logz_jac,
                       const double *__restrict__ ssq_new) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= A.n / 2) return;
  int64_t other;
  const int64_t j = ens_mover(A, t, other);
  double x[D], us, log_ua;
  int r;
#pragma unroll
  for (int p = 0; p < D; ++p) x[p] = A.q[j * D + p];
  const double lx = A.l[j];
  ens_draws(A, (uint64_t)(A.offset + j), A.iter, us, log_ua, r);
  const int found = !ens_healthy<D>(A, x, lx) ? ENS_STUCK : (inbox[j] != 0 ? ENS_INSIDE : ENS_OUTSIDE);
  bool acc = false;
  if (found == ENS_INSIDE) {
    const double ln = ens_logtarget(ssq_new[j], A.shape);
    acc = ens_decide(logz_jac[j], lx, ln, log_ua);
    if (acc) {
#pragma unroll
      for (int p = 0; p < D; ++p) A.q[j * D + p] = q_new[j * D + p];
      A.l[j] = ln;
    }
  }
  ens_count(A, j, found, acc);
}

// ---- the solve of one half-step alone ----------------------------------------------------------------------------------------------------
// ssq_new[j] = SSq(q_new[j]) for the movers j of half A.half whose inbox is 1, in ensemble_move_kernel's OWN arrangement: one workgroup
// per island, lane i solves mover i's proposal, a lane without one rides along with the same harmless point and a WAVE without one
// skips the solve.  The lockstep driver's tier decisions are wave-wide, so a trajectory's last bits depend on the lanes it shares a
// wave with: only this arrangement gives the split path the fused kernel's bits (rsf_fit_normal's waves hold other trajectories).
template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) ensemble_ssq_kernel(Consts K, EnsArgs A, const double *__restrict__ q_new,
                                                                            const uint8_t *__restrict__ inbox, double *__restrict__ ssq_new) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int B = (int)blockDim.x;
  const int64_t base = (int64_t)blockIdx.x * (2 * (int64_t)B);
  if (A.group_walkers > 0) K.data += (base / A.group_walkers) * K.nout;
  const double *ld = lds + rsf::lds_data_offset(K);
  const int64_t j = base + (int64_t)A.half * B + threadIdx.x;
  const bool inb = inbox[j] != 0;
  double pq[3] = {1000.0, K.a_def, K.b_def};
  if (inb) {
    pq[0] = q_new[j * D];
    if constexpr (D == 3) { pq[1] = q_new[j * D + 1]; pq[2] = q_new[j * D + 2]; }
  }
  const bool solve = __any(inb) != 0;  // wave-uniform
  const rsf::Lane L = rsf::make_lane<DAMP>(pq[0], pq[1], pq[2], K);
  rsf::State st = rsf::initial_state(pq[0], L, K);
  double ssq = 0.0;
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    rsf::stage_chunk(lds, K, k0, kn);
    if (k0 == 1) {
      const double d0 = lds[rsf::lds_d0_offset(K)];
      ssq = d0 * d0;
    }
    if (solve)
      rsf::integrate_lockstep<DAMP>(lds, K, L, st, kn, [&](double ak, int ko) { const double rr = ak - ld[ko]; ssq = __builtin_fma(rr, rr, ssq); }, [] {});
  }
  if (inb) ssq_new[j] = ssq;
}

// ---- the fused hot path -------------------------------------------------------------------------------------------------------------
// One workgroup of B = blockDim.x lanes owns island blockIdx.x; lane i carries walker i of half 0 and walker i of half 1 and solves in
// both half-steps, A.n_iter iterations (2 A.n_iter half-steps) inside the launch.  A half-step: every lane publishes its walker of
// the RESTING half into an LDS area of B D doubles behind the table chunk, a barrier, the mover gathers its partner from that area,
// then smc_move_kernel's solve — rsf::integrate_lockstep with the sum of squares kept per lane in the per-sample hook, the table and
// the observation staged chunk by chunk (rsf::stage_chunk) — and the decision.  The next half-step's publish is separated from
// this one's gathers by stage_chunk's barriers (a solve stages at least one chunk, and every lane takes part in the staging).
// A stuck walker or one whose proposal left the box rides along with a harmless point; a WAVE without a proposal inside the box
// skips the solve but none of the barriers.
// The resting half's state is NOT parked in LDS or held in registers: it lives in q and l in global memory, which the owning lane
// wrote itself one half-step earlier, and is loaded again when it moves (D + 1 loads per solve).  Across the solve only the
// mover's proposal, l, J and log U_a are live, so the kernel keeps smc_move_kernel's register budget.
template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) ensemble_move_kernel(Consts K, EnsArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int B = (int)blockDim.x;
  const int64_t base = (int64_t)blockIdx.x * (2 * (int64_t)B);
  if (A.group_walkers > 0) K.data += (base / A.group_walkers) * K.nout;  // an island's walkers share one observation series
  const double *ld = lds + rsf::lds_data_offset(K);
  double *pub = lds + rsf::lds_d0_offset(K) + 1;
  for (int hs = 0; hs < 2 * A.n_iter; ++hs) {  // ONE loop over the half-steps: the solve is compiled once
    const int it = hs >> 1, h = hs & 1;
    const int64_t j = base + (int64_t)h * B + threadIdx.x, o = base + (int64_t)(1 - h) * B + threadIdx.x;
#pragma unroll
    for (int p = 0; p < D; ++p) pub[threadIdx.x * D + p] = A.q[o * D + p];
    __syncthreads();
    double x[D], xn[D], us, log_ua, J = 0.0;
    int r;
#pragma unroll
    for (int p = 0; p < D; ++p) x[p] = A.q[j * D + p];
    const double lx = A.l[j];
    ens_draws(A, (uint64_t)(A.offset + j), A.iter + (uint32_t)it, us, log_ua, r);
    int found = ENS_STUCK;
    if (ens_healthy<D>(A, x, lx)) {
      double y[D];
#pragma unroll
      for (int p = 0; p < D; ++p) y[p] = pub[r * D + p];
      found = ens_proposal<D>(A, us, x, y, xn, J) ? ENS_INSIDE : ENS_OUTSIDE;
    }
    const bool inb = found == ENS_INSIDE;
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
        rsf::integrate_lockstep<DAMP>(lds, K, L, st, kn, [&](double ak, int ko) { const double rr = ak - ld[ko]; ssq = __builtin_fma(rr, rr, ssq); }, [] {});
    }
    const double ln = ens_logtarget(ssq, A.shape);
    const bool acc = inb && ens_decide(J, lx, ln, log_ua);
    if (acc) {
#pragma unroll
      for (int p = 0; p < D; ++p) A.q[j * D + p] = xn[p];
      A.l[j] = ln;
    }
    ens_count(A, j, found, acc);
    if (A.tq) {
      const int64_t row = (int64_t)it * A.n + j;
#pragma unroll
      for (int p = 0; p < D; ++p) A.tq[row * D + p] = acc ? xn[p] : x[p];
      A.tl[row] = acc ? ln : lx;
    }
  }
}

}  // namespace rsfk
