// rsf_kernels_core.h — the model's and the chains' kernels: forward_kernel, init_kernel / init_dp_kernel, ssq32_kernel,
// propose_kernel, transpose_kernel and the probe_philox / probe_draws self-test kernels.  Included by rsf_hip.hip only (transpose_kernel and
// the probes are not templates), and by tools/ that build one kernel alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rsf_kernel_common.h"
#include "rsf_device_dop853.h"
#include "rsf_device_f32.h"

namespace rsfk {

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
template <bool DAMP, bool WANT_SSQ, bool WANT_ACC, int MODE>
__global__ void __launch_bounds__(kMaxBlock)
forward_kernel(Consts K, int64_t n, const double *__restrict__ dc, const double *__restrict__ a,
               const double *__restrict__ b, double *__restrict__ ssq_out, double *__restrict__ acc_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  const double dci = active ? dc[i] : 1.0;
  const double ai = (active && a) ? a[i] : K.a_def;
  const double bi = (active && b) ? b[i] : K.b_def;
  double *acc_i = WANT_ACC ? acc_out + i : nullptr;
  const bool resident = K.nchunks == 1;
  double ssq;
  if constexpr (MODE == RK4_F32) {
    float *lds32 = reinterpret_cast<float *>(lds);
    if (resident) rsf::f32::stage_chunk32(lds32, K, 1, K.nout - 1);
    ssq = rsf::f32::solve32<DAMP, WANT_SSQ, WANT_ACC>(lds32, K, resident, active, dci, ai, bi, acc_i, n);
  } else {
    if constexpr (MODE == DOP853) {
      if (resident) rsf::dp::stage_chunk_dp(lds, K, 1, K.nout - 1);
      ssq = rsf::dp::solve<DAMP, WANT_SSQ, WANT_ACC>(lds, K, resident, active, dci, ai, bi, acc_i, n);
    } else {
      if (resident) rsf::stage_chunk(lds, K, 1, K.nout - 1);
      rsf::Wave W;  // every lane's result is wanted: no early rejection (thr = +inf), statistics unused
      ssq = rsf::solve<DAMP, WANT_SSQ, WANT_ACC, 2 * rsf::kTightUnroll>(lds, K, resident, active, dci, ai, bi, INFINITY, acc_i, n, W);
    }
  }
  if (WANT_SSQ && active) ssq_out[i] = ssq;
}

struct InitArgs {
  int64_t C;
  double fd;       // forward-difference relative step, MCMC.py:251
  double inv_dof;  // 1 / (nout - len(qpriors)), MCMC.py:261
  double width[RSF_MAX_PARAMS];  // hi - lo of the prior box (three-parameter chains: initial_covariance)
  const double *q0;  // [d][C]
  double *ssq, *std2, *V;  // [C], [C], [d*d][C]
};

// The initial proposal covariance from the sensitivities' Gram matrix X^T X and sigma^2_0.
// One parameter — the reference's sampler: Vstart = sigma^2 (X^T X)^-1, MCMC.py:265-266, as it stands.
// Three parameters (Dc, a, b) — this build's extension (BASELINE config 5), where that formula does not give a proposal:
// the series depends on Dc and a almost only through their product (relative sensitivities equal to five digits, correlation
// eigenvalue 2e-11) and hardly at all on b (3000 times smaller), so (X^T X)^-1 is astronomically wide along a ridge — and
// what little it says there is forward-difference rounding.  The data do not identify those directions; the PRIOR does.  So
// the box prior enters the way a Gaussian of the same variance would, in coordinates u_p = (q_p - lo_p) / w_p that make the box a
// unit cube:        M = W (X^T X) W / sigma^2 + 12 I,      V = W M^-1 W,      W = diag(w_p = hi_p - lo_p)
// (a uniform variable on a unit interval has variance 1/12).  M is symmetric positive definite with every eigenvalue >= 12
// (condition number ~4e3 at the BASELINE problem): no guard, no fallback.  Identified directions get their Gauss-Newton
// width, unidentified ones the width of the box.
template <int D>
__device__ __forceinline__ void initial_covariance(const double *xtx, double std2, const double *width, double *V) {
  if constexpr (D == 1) {
    V[0] = std2 * (1.0 / xtx[0]);
  } else {
    double M[D * D], Mi[D * D];
    const double is2 = 1.0 / std2;
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
      for (int r = 0; r < D; ++r) M[p * D + r] = (width[p] * xtx[p * D + r] * width[r]) * is2 + (p == r ? 12.0 : 0.0);
    rsf::sym_inverse<D>(M, Mi);
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
      for (int r = 0; r < D; ++r) V[p * D + r] = width[p] * Mi[p * D + r] * width[r];
  }
}

// compute_initial_covariance + the initial SSq (MCMC.py:244-266, 468): ONE LANE PER TRAJECTORY.  A chain owns a group of
// G = D + 1 adjacent lanes (a pair for one parameter, a quad for three): lane 0 of the group integrates the chain's start
// point, lane p + 1 the point with parameter p moved by the forward-difference step (MCMC.py:251) — each with the sampler's
// own straight-line tier code and nothing but the forward kernel's registers.  Where an output sample completes, the
// group's lanes exchange their acceleration samples by lane shuffles: every lane forms its sensitivity against lane 0's
// sample (perturbed value in the denominator, MCMC.py:264), lane 0 collects them and accumulates the residual and X^T X,
// sample by sample, without storing trajectories.  (Until round 4 ONE lane carried all 1 + D trajectories in lockstep: four
// sets of lane constants and states, 256 VGPRs + 42-120 AGPRs of spills, one wave per SIMD.)
// The acceleration sample is cv * (sum of the interval's weighted V-derivative sums), like the sampler's (rsf::emit_incr):
// the initial SSq is the value the sampler computes for the same point to rounding, and the difference of two trajectories'
// samples — which a relative step of 1e-6 amplifies a million-fold — does not go through two velocities near V_ref.
template <int D>
struct InitGroup {
  static constexpr int G = D + 1;  // lanes per chain: 2 or 4, a power of two, so a group never straddles a wave
  const unsigned t = threadIdx.x;
  const int tr = (int)(t & (G - 1));                                              // which trajectory of its chain this lane integrates
  const int64_t chain = (int64_t)blockIdx.x * (blockDim.x / G) + (t / G);
  const int lane0 = (int)((t & 63) & ~(unsigned)(G - 1));                         // the group's first lane within the wave
  double xtx[D * D], ssq = 0.0;

  __device__ __forceinline__ InitGroup() {
#pragma unroll
    for (int e = 0; e < D * D; ++e) xtx[e] = 0.0;
  }
  // the observation series of the workgroup's chain group (all of a workgroup's chains belong to one)
  __device__ __forceinline__ void select_group(Consts &K) const {
    if (K.group_chains > 0) K.data += (((int64_t)blockIdx.x * (blockDim.x / G)) / K.group_chains) * K.nout;
  }
  // this lane's parameter vector (Dc, a, b) and, for a perturbed trajectory, 1 / (perturbed value * step)
  __device__ __forceinline__ void parameters(const Consts &K, const InitArgs &A, bool active, double (&pq)[3], double &inv_den) const {
    pq[0] = 1000.0; pq[1] = K.a_def; pq[2] = K.b_def;
    if (active) {
      pq[0] = A.q0[chain];
      if (D == 3) { pq[1] = A.q0[A.C + chain]; pq[2] = A.q0[2 * A.C + chain]; }
    }
    inv_den = 0.0;
#pragma unroll
    for (int p = 0; p < D; ++p)
      if (tr == p + 1) {
        pq[p] = pq[p] * (1 + A.fd);
        inv_den = 1.0 / (pq[p] * A.fd);  // perturbed value in the denominator, MCMC.py:264
      }
  }
  // the value lane `SRC` of this lane's group holds.  A group is an aligned pair or quad of lanes, so this is a DPP quad_perm move
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
  // an output sample is complete: ak = this lane's acceleration sample, obs the observation (every lane of the group calls, in
  // converged control flow).  Only the upper triangle of X^T X is accumulated; finish() mirrors it
  __device__ __forceinline__ void sample(double ak, double obs, double inv_den) {
    const double ak0 = from_lane<0>(ak);
    const double x = (ak - ak0) * inv_den;  // lane p + 1: the sensitivity to parameter p; lane 0: 0
    double xs[D];
    gather<0>(x, xs);
    const double r = ak - obs;  // meaningful in lane 0 (the others accumulate values nobody reads)
    ssq = __builtin_fma(r, r, ssq);
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
      for (int r2 = p; r2 < D; ++r2) xtx[p * D + r2] = __builtin_fma(xs[p], xs[r2], xtx[p * D + r2]);
  }
  __device__ __forceinline__ void finish(const InitArgs &A, bool active) const {
    if (active && tr == 0) {
      const double std2 = ssq * A.inv_dof;
      double V[D * D], M[D * D];
#pragma unroll
      for (int p = 0; p < D; ++p)
#pragma unroll
        for (int r2 = 0; r2 < D; ++r2) M[p * D + r2] = xtx[p <= r2 ? p * D + r2 : r2 * D + p];
      initial_covariance<D>(M, std2, A.width, V);
#pragma unroll
      for (int e = 0; e < D * D; ++e) A.V[e * A.C + chain] = V[e];  // MCMC.py:266
      A.std2[chain] = std2;
      A.ssq[chain] = ssq;
    }
  }
};

template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) init_kernel(Consts K, InitArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  InitGroup<D> grp;
  grp.select_group(K);
  const bool active = grp.chain < A.C;
  double pq[3], inv_den;
  grp.parameters(K, A, active, pq, inv_den);
  const rsf::Lane L = rsf::make_lane<DAMP>(pq[0], pq[1], pq[2], K);
  rsf::State st = rsf::initial_state(pq[0], L, K);
  if (active) { const double d0 = K.data[0]; grp.ssq = d0 * d0; }
  const double *ld = lds + rsf::lds_data_offset(K);
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    rsf::stage_chunk(lds, K, k0, kn);
    rsf::integrate_lockstep<DAMP>(lds, K, L, st, kn, [&](double ak, int ko) { grp.sample(ak, ld[ko], inv_den); }, [] {});
  }
  grp.finish(A, active);
}

// compute_initial_covariance + initial SSq in the reference's DOP853 scheme, one lane per trajectory like init_kernel: every
// lane takes its own dop853 calls interval by interval (its own carried step size); the group's lanes meet at every
// output sample.
template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) init_dp_kernel(Consts K, InitArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  InitGroup<D> grp;
  grp.select_group(K);
  const bool active = grp.chain < A.C;
  double pq[3], inv_den;
  grp.parameters(K, A, active, pq, inv_den);
  const rsf::dp::LaneD L = rsf::dp::make_lane_dp(pq[0], pq[1], pq[2]);
  rsf::dp::Carry cw = rsf::dp::fresh_carry();
  double y[3] = {K.mu0, pq[0] / K.V_ref, K.V_ref}, x = K.t0, vprev = K.V_ref;
  bool failed = false;
  if (active) { const double d0 = K.data[0]; grp.ssq = d0 * d0; }
  const double *ld = lds + rsf::dp::lds_data_offset_dp(K);
  const double delta_t = K.dt;
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    rsf::dp::stage_chunk_dp(lds, K, k0, kn);
    for (int kk = 0; kk < kn; ++kk) {
      double ak = 0.0;  // a trajectory whose integrator failed leaves zeros, like the reference (RateStateModel.py:361-366, 381)
      if (!failed) {
        failed = !rsf::dp::call<DAMP>(K, L, lds + rsf::dp::kTab * kk, x, x + delta_t, y, cw, true);
        ak = (y[2] - vprev) * K.inv_dt;
        vprev = y[2];
      }
      grp.sample(ak, ld[kk], inv_den);
    }
  }
  grp.finish(A, active);
}

// float32 mode: the sampler compares sums of squares from float32 solves, so the initial SSq (computed by the
// float64 init kernel together with the float64-only sensitivities) is replaced by its float32 value.
template <int D, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock) ssq32_kernel(Consts K, int64_t C, const double *q, double *ssq) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  rsf::select_group(K);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < C;
  const double dc = active ? q[i] : 1.0;
  const double a = (active && D == 3) ? q[C + i] : K.a_def, b = (active && D == 3) ? q[2 * C + i] : K.b_def;
  const double s = rsf::f32::solve32<DAMP, true, false>(reinterpret_cast<float *>(lds), K, false, active, dc, a, b, nullptr, 0);
  if (active) ssq[i] = s;
}

// rsf_mcmc_propose: the proposal the next iteration of mcmc_kernel will make from z, and whether it is inside the box
struct ProposeArgs {
  int64_t C;
  const double *q, *V;  // [d][C], [d*d][C]
  const double *z;      // [C][d]
  double lo[RSF_MAX_PARAMS], hi[RSF_MAX_PARAMS];
  double *qn;           // [C][d]
  uint8_t *inb;         // [C]
};

template <int D>
__global__ void __launch_bounds__(kMaxBlock) propose_kernel(ProposeArgs A) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.C) return;
  double q[D], V[D * D], Lf[D * D], z[D], qn[D];
#pragma unroll
  for (int p = 0; p < D; ++p) { q[p] = A.q[p * A.C + i]; z[p] = A.z[i * D + p]; }
#pragma unroll
  for (int e = 0; e < D * D; ++e) V[e] = A.V[e * A.C + i];
  rsf::chol_lower<D>(V, Lf);
  double tri[D * (D + 1) / 2];
  int e = 0;
#pragma unroll
  for (int p = 0; p < D; ++p)
#pragma unroll
    for (int r = 0; r <= p; ++r) tri[e++] = Lf[p * D + r];
  propose<D>(q, [&](int k) { return tri[k]; }, z, qn);
#pragma unroll
  for (int p = 0; p < D; ++p) A.qn[i * D + p] = qn[p];
  A.inb[i] = in_box<D>(qn, A) ? 1 : 0;
}

// [n][d] <-> [d][n] between the C ABI's per-chain layout and the kernels' structure of arrays (d = 3 only; for one
// parameter the two coincide)
__global__ void __launch_bounds__(kMaxBlock) transpose_kernel(int64_t n, int d, const double *__restrict__ src, double *__restrict__ dst, bool to_soa) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int e = 0; e < d; ++e) {
    if (to_soa) dst[(int64_t)e * n + i] = src[i * d + e];
    else dst[i * d + e] = src[(int64_t)e * n + i];
  }
}

// out[0..3] = philox words (as doubles are not used here): layout documented at the call sites
__global__ void probe_philox_kernel(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                    uint32_t *out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    uint32_t w[4];
    rsf::philox4x32_10(c0, c1, c2, c3, k0, k1, w);
    for (int j = 0; j < 4; ++j) out[j] = w[j];
  }
}

// out = { z0, z1, z2, u, g }
__global__ void probe_draws_kernel(uint64_t seed, uint64_t chain, uint32_t iter, int d, double shape, double *out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    uint32_t w[4];
    double z[4] = {0, 0, 0, 0};
    rsf::draw_words(seed, chain, iter, rsf::SLOT_Z01, w);
    rsf::normal_pair(w, z[0], z[1]);
    if (d > 2) { rsf::draw_words(seed, chain, iter, rsf::SLOT_Z2, w); rsf::normal_pair(w, z[2], z[3]); }
    rsf::draw_words(seed, chain, iter, rsf::SLOT_U, w);
    out[0] = z[0]; out[1] = z[1]; out[2] = z[2];
    out[3] = rsf::u53(w[0], w[1]);
    out[4] = rsf::gamma_draw(seed, chain, iter, shape - 1.0 / 3.0, 1.0 / sqrt(9.0 * (shape - 1.0 / 3.0)));
  }
}

}  // namespace rsfk
