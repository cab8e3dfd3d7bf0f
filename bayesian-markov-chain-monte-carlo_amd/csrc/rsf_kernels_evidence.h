// rsf_kernels_evidence.h — the marginal likelihood of the pooled draws by bridge sampling (include/rsf_evidence.h):
// evidence_propose_kernel, evidence_logg_kernel, evidence_logtarget_kernel, evidence_terms_kernel.  Included by rsf_evidence.hip
// only.  The last step of the sums, over the workgroups' partials, is rsfh::sum_strided_tree (rsf_host.h).
//
// Reproducibility: every sum below has an order fixed by the shape of the input and the launch geometry, which the host derives
// from n alone — per thread in index order, per wave by the shuffle tree, the waves of a workgroup and the workgroups' partials in
// index order.  No floating-point atomic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_evidence.h"
#include "rsf_kernel_common.h"
#include "rsf_device.h"

namespace rsfk {

constexpr int kEvBlocks = 1024;  // workgroups of evidence_terms_kernel at most: four per CU
constexpr int kEvFields = 4;     // per set: terms counted, terms left out (-inf), sum t, sum t^2

// the Gaussian proposal and the box: a kernel argument, so that every entry is a scalar register
struct EvGauss {
  double m[RSF_EVIDENCE_MAX_PARAMS];
  double L[RSF_EVIDENCE_MAX_PARAMS * (RSF_EVIDENCE_MAX_PARAMS + 1) / 2];  // row-major lower triangle
  double logc;                                                            // -sum log L_pp - d/2 log(2 pi)
  double lo[RSF_EVIDENCE_MAX_PARAMS], hi[RSF_EVIDENCE_MAX_PARAMS];
  int32_t tr[RSF_EVIDENCE_MAX_PARAMS];                                    // 1: phi_p = log q_p
};

// log g(phi) — the ONE density code of rsf_evidence_propose and rsf_evidence_logg: y = L^-1 (phi - m) by forward substitution
template <int D>
__device__ __forceinline__ double ev_logg(const double (&phi)[D], const EvGauss &G) {
  double y[D], ss = 0.0;
  int e = 0;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    double s = phi[p] - G.m[p];
#pragma unroll
    for (int r = 0; r < p; ++r) s = __builtin_fma(-G.L[e++], y[r], s);
    y[p] = s / G.L[e++];
    ss = __builtin_fma(y[p], y[p], ss);
  }
  return __builtin_fma(-0.5, ss, G.logc);
}

struct EvProposeArgs {
  int64_t n, offset;
  uint64_t seed;
  double *theta, *logg;  // [n][D], [n]
  uint8_t *inbox;        // [n]
};

template <int D>
__global__ void __launch_bounds__(kMaxBlock) evidence_propose_kernel(EvGauss G, EvProposeArgs A) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.n) return;
  // the normals of (seed, chain = offset + j, iteration 0), as probe_draws_kernel reports them (rsf_mcmc_draws)
  uint32_t w[4];
  double z[4] = {0, 0, 0, 0};
  rsf::draw_words(A.seed, (uint64_t)(A.offset + j), 0u, rsf::SLOT_Z01, w);
  rsf::normal_pair(w, z[0], z[1]);
  if (D > 2) { rsf::draw_words(A.seed, (uint64_t)(A.offset + j), 0u, rsf::SLOT_Z2, w); rsf::normal_pair(w, z[2], z[3]); }
  double m[D], phi[D], th[D];
#pragma unroll
  for (int p = 0; p < D; ++p) m[p] = G.m[p];
  propose<D>(m, [&](int k) { return G.L[k]; }, z, phi);
#pragma unroll
  for (int p = 0; p < D; ++p) {
    th[p] = G.tr[p] ? exp(phi[p]) : phi[p];
    A.theta[j * D + p] = th[p];
  }
  A.logg[j] = ev_logg<D>(phi, G);
  A.inbox[j] = in_box<D>(th, G) ? 1 : 0;
}

template <int D>
__global__ void __launch_bounds__(kMaxBlock) evidence_logg_kernel(EvGauss G, int64_t n, const double *__restrict__ theta, double *__restrict__ logg) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double phi[D];
#pragma unroll
  for (int p = 0; p < D; ++p) {
    const double t = theta[i * D + p];
    phi[p] = G.tr[p] ? (t > 0.0 ? log(t) : __longlong_as_double(0x7ff8000000000000ll)) : t;
  }
  logg[i] = ev_logg<D>(phi, G);
}

// ---- the fused hot path -------------------------------------------------------------------------------------------------
struct EvTargetArgs {
  int64_t n;
  const double *theta, *logg;  // [n][D], [n]
  double *l;                   // [n]
  double shape;
  double lo[RSF_EVIDENCE_MAX_PARAMS], hi[RSF_EVIDENCE_MAX_PARAMS];
  int32_t tr[RSF_EVIDENCE_MAX_PARAMS];
};

// One lane per point, the float64 RK4 tier code driven by rsf::integrate_lockstep like init_kernel and predict_kernel, with the
// sum of squares against the observation (staged with the loading table: rsf::stage_chunk) kept per lane as the samples
// complete.  A lane outside the box, or past the last point, rides along with a harmless point; a WAVE without a lane inside the
// box skips the solve (it still takes part in the staging, whose barriers are the workgroup's).
template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) evidence_logtarget_kernel(Consts K, EvTargetArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < A.n;
  double th[D];
#pragma unroll
  for (int p = 0; p < D; ++p) th[p] = active ? A.theta[i * D + p] : 0.5 * (A.lo[p] + A.hi[p]);
  const bool inb = active && in_box<D>(th, A);
  double jac = 0.0;
#pragma unroll
  for (int p = 0; p < D; ++p) jac += (A.tr[p] && inb) ? log(th[p]) : 0.0;
  double pq[3] = {1000.0, K.a_def, K.b_def};
  if (inb) {
    pq[0] = th[0];
    if constexpr (D == 3) { pq[1] = th[1]; pq[2] = th[2]; }
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
  if (active) {
    const bool ok = inb && __builtin_isfinite(ssq) && ssq > 0.0;
    A.l[i] = ok ? __builtin_fma(-A.shape, log(ssq), jac) - A.logg[i] : -INFINITY;
  }
}

// ---- one bridge iteration's sums ------------------------------------------------------------------------------------------
// NUM: the proposal draws' terms t2 = e^a / (s1 e^a + s2 r); else the posterior draws' t1 = 1 / (s1 e^b + s2 r).  Each is formed
// through the exponential of -|.|, so that a spread of 1e4 about lstar gives 0 or the bound, never inf / inf.
// part[block][kEvFields] = [terms counted, terms left out (l = -inf), sum t, sum t^2]; a NaN or +inf entry (and for the posterior
// draws -inf) makes the counts disagree with n: the host refuses the call.
template <bool NUM>
__global__ void __launch_bounds__(kMaxBlock)
evidence_terms_kernel(int64_t n, const double *__restrict__ l, double lstar, double s1, double s2r, double *__restrict__ part) {
  __shared__ double sh[kMaxBlock / 64][kEvFields];
  double s[kEvFields] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = l[i], a = v - lstar;
    const bool fin = __builtin_isfinite(v), out = NUM && v == -INFINITY;
    const double e = exp(-fabs(a));  // in (0, 1], 0 by underflow
    double t;
    if (NUM) t = a > 0.0 ? 1.0 / __builtin_fma(s2r, e, s1) : e / __builtin_fma(s1, e, s2r);
    else t = a > 0.0 ? e / __builtin_fma(s2r, e, s1) : 1.0 / __builtin_fma(s1, e, s2r);
    t = fin ? t : 0.0;
    s[0] += fin ? 1.0 : 0.0;
    s[1] += out ? 1.0 : 0.0;
    s[2] += t;
    s[3] = __builtin_fma(t, t, s[3]);
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int f = 0; f < kEvFields; ++f) {
    const double v = wave_sum(s[f]);
    if ((threadIdx.x & 63) == 0) sh[wave][f] = v;
  }
  __syncthreads();
  block_fields_store(sh, kEvFields, part, (int64_t)blockIdx.x * kEvFields);
}

}  // namespace rsfk
