// rsf_kernels_law_grid.h — the exact posterior of a state-law model on a tensor grid in the coordinates of a fit
// (include/rsf_law_grid.h): law_grid_point, the node of a flat index; law_logtarget_kernel, the fused hot path; and
// law_grid_moments_kernel, the moments in natural coordinates.  Included by rsf_law_grid.hip only.  The step is
// rsf_kernels_law.h's law_step, the sample and its residual rsf_kernels_observe.h's observe_sample, called from here, not restated.
//
// Reproducibility: every sum below has an order fixed by the shape of the grid — per thread in node order, per wave by the
// shuffle tree, the waves of a workgroup in index order.  No floating-point atomic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_law_grid.h"
#include "rsf_kernels_observe.h"

namespace rsfk {

// Register budget of law_logtarget_kernel: three workgroups per CU, i.e. three waves per SIMD (at most 168 registers), law_fit_kernel's
// and grid_logtarget_kernel's bracket.  The eight instances take 112 to 118 registers under it and none has scratch
// (profiles/law_grid/resource_report.txt): the bound costs nothing; the LDS of the table chunk, not the registers, decides how
// many workgroups a CU holds.
constexpr int kLawGridBlocks = 3;

// the axes of one call: a kernel argument, so that every entry is a scalar register.  z and w point at device copies; an axis the
// grid lacks has n = 1 and one node 0 of weight 1 (rsf_kernels_grid.h's GridAxes, which only rsf_grid.hip may include)
struct LawGridAxes {
  int32_t n[RSF_LAW_GRID_MAX_PARAMS];
  const double *z[RSF_LAW_GRID_MAX_PARAMS], *w[RSF_LAW_GRID_MAX_PARAMS];
};

// the affine map phi = m + L z and what each phi_p is: a kernel argument, so that every entry is a scalar register
struct LawGridMap {
  double m[RSF_LAW_GRID_MAX_PARAMS];
  double L[RSF_LAW_GRID_MAX_PARAMS * (RSF_LAW_GRID_MAX_PARAMS + 1) / 2];  // row-major lower triangle
  int32_t tr[RSF_LAW_GRID_MAX_PARAMS];                                    // 1: q = exp(phi_p)
  int32_t perm[RSF_LAW_GRID_MAX_PARAMS];                                  // phi_p is parameter perm[p] of (Dc, a, b)
};

// s + e <- (s + e) + L z, carried as an unevaluated sum: the product split exactly by one fma, the sum by Knuth's TwoSum.  Contraction
// is off, so that the sum's steps stay the roundings the error term accounts for.
__device__ __forceinline__ void law_grid_add(double &s, double &e, double L, double z) {
#pragma clang fp contract(off)
  const double ph = L * z, pl = __builtin_fma(L, z, -ph);
  const double t = s + ph, bb = t - s;
  e += ((s - (t - bb)) + (ph - bb)) + pl;
  s = t;
}

// The node of the flat index ii = i0 + n0 (i1 + n1 i2) (grid_logtarget_kernel's decomposition), the ONE formation of both kernels:
//   s + e  = m_p + sum_{r <= p} L_pr z_r   in the order r = 0 .. p, carried as an unevaluated sum (law_grid_add): a window that
//            reaches far from the fit's point cancels m_p against L z, and a plain fma chain would keep the absolute rounding
//            error of its largest partial sum, which is no bound in ulp of the node
//   phi_p  = s + e, one rounding; its error err_p = (s - phi_p) + e is kept
//   q      = phi_p, or exp(phi_p) + exp(phi_p) err_p (one fma) where tr_p: the rounding of phi_p would otherwise be a RELATIVE error
//            of q, |phi_p| / 2 ulp of it (log a = -4.5: more than two ulp before the exponential's own)
// q[perm[p]] takes it.  iz: (i0, i1, i2).  The Jacobian of the logged parameters is formed by law_logtarget_kernel, from q.
template <int D>
__device__ __forceinline__ void law_grid_point(const LawGridAxes &G, const LawGridMap &M, uint32_t ii, double (&q)[3], uint32_t (&iz)[3]) {
  double z[D];
  if constexpr (D == 1) {
    iz[0] = ii; iz[1] = 0u; iz[2] = 0u;
    z[0] = G.z[0][ii];
  } else {
    const uint32_t n0 = (uint32_t)G.n[0], n1 = (uint32_t)G.n[1];
    const uint32_t r = ii / n0, i0 = ii - r * n0, i2 = r / n1, i1 = r - i2 * n1;
    iz[0] = i0; iz[1] = i1; iz[2] = i2;
    z[0] = G.z[0][i0];
    z[1] = G.z[1][i1];
    z[2] = G.z[2][i2];
  }
  int e = 0;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    double s = M.m[p], c = 0.0;
#pragma unroll
    for (int r = 0; r <= p; ++r) law_grid_add(s, c, M.L[e++], z[r]);
    const double phi = s + c, err = (s - phi) + c;
    double v = phi;
    if (M.tr[p]) {  // wave-uniform
      const double ex = exp(phi);
      v = __builtin_fma(ex, err, ex);
    }
    // perm is wave-uniform; written as selects so that q stays in registers
    const int k = D == 1 ? 0 : M.perm[p];
    q[0] = k == 0 ? v : q[0];
    q[1] = k == 1 ? v : q[1];
    q[2] = k == 2 ? v : q[2];
  }
}

// ---- the fused hot path -------------------------------------------------------------------------------------------------
struct LawTargetArgs {
  int64_t N;
  LawGridAxes G;
  LawGridMap M;
  const double *theta, *logg;  // [N][D], [N]: the points and what is subtracted; theta NULL: the grid (wave-uniform)
  double *l, *ssq, *q_out;     // [N], [N], [N][D] or NULL
  double shape;
  double lo[RSF_LAW_GRID_MAX_PARAMS], hi[RSF_LAW_GRID_MAX_PARAMS];  // of (Dc, a, b)
};

// One lane per point, law_observe_kernel's solve with the running SSq (sample 0 included) in law_dr_solve's arrangement: a lane
// outside the CLOSED box, or past N, rides along with the harmless point (1000, a_def, b_def); a WAVE without a lane inside skips
// the steps — and only the steps: stage_chunk's barriers are taken by every wave of the workgroup.  No atomics, no scratch, no
// tier, no guard: a NaN trajectory runs to its end and gives l = -inf.
template <int D, int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock, kLawGridBlocks) law_logtarget_kernel(Consts K, int32_t observable, LawTargetArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < A.N;
  const bool points = A.theta != nullptr;  // wave-uniform
  double q[3] = {1000.0, K.a_def, K.b_def}, jac = 0.0;
  if (points) {
#pragma unroll
    for (int p = 0; p < D; ++p) q[p] = active ? A.theta[i * D + p] : 0.5 * (A.lo[p] + A.hi[p]);
  } else {
    uint32_t iz[3];
    law_grid_point<D>(A.G, A.M, active ? (uint32_t)i : 0u, q, iz);
  }
  bool inb = active;
#pragma unroll
  for (int p = 0; p < D; ++p) inb = inb && (q[p] >= A.lo[p]) && (q[p] <= A.hi[p]);  // closed: a node on a face carries a weight
  // evidence_logtarget_kernel's Jacobian, for both sources: the logarithm of the logged parameters of a point inside, in the order
  // p = 0 .. D - 1.  At a node log q_p is phi_p to the rounding of exp and log (an absolute 1e-16 beside |l| of 1e3); taken from q, a
  // node given back as a point has the same l bit for bit.
#pragma unroll
  for (int p = 0; p < D; ++p) {
    const int k = D == 1 ? 0 : A.M.perm[p];
    const double t = k == 0 ? q[0] : (k == 1 ? q[1] : q[2]);
    jac += (A.M.tr[p] && inb) ? log(t) : 0.0;
  }
  if (A.q_out && active) {
#pragma unroll
    for (int p = 0; p < D; ++p) A.q_out[i * D + p] = q[p];
  }
  double pq[3] = {1000.0, K.a_def, K.b_def};
  if (inb) {
    pq[0] = q[0];
    if constexpr (D == 3) { pq[1] = q[1]; pq[2] = q[2]; }
  }
  const bool solve = __any(inb) != 0;  // wave-uniform
  const rsf::Lane L = rsf::make_lane<DAMP>(pq[0], pq[1], pq[2], K);
  const rsf::State s0 = rsf::initial_state(pq[0], L, K);
  double ms = s0.ms, x = s0.x, V = s0.V, vprev = s0.V, ssq = 0.0;
  // law_observe_kernel's per-lane factor and sample 0, restated as law_dr_solve restates them
  const double scale = observable == RSF_OBS_THETA ? pq[0] * K.inv_vref : L.kprime;
  const double first = observable == RSF_OBS_ACC ? 0.0 : observable == RSF_OBS_VELOCITY ? s0.V : observable == RSF_OBS_MU ? scale * s0.ms : s0.x * scale;
  const double *ld = lds + rsf::lds_data_offset(K);
  int phase = 0;  // RK4 steps since the last output sample (wave-uniform)
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    rsf::stage_chunk(lds, K, k0, kn);
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
  if (active) {
    const bool ok = inb && __builtin_isfinite(ssq) && ssq > 0.0;
    const double g = A.logg ? A.logg[i] : 0.0;
    A.l[i] = ok ? __builtin_fma(-A.shape, log(ssq), jac) - g : -INFINITY;
    A.ssq[i] = inb ? ssq : __longlong_as_double(0x7ff8000000000000ll);
  }
}

// ---- the moments in natural coordinates ---------------------------------------------------------------------------------------
struct LawMomentArgs {
  LawGridAxes G;
  LawGridMap M;
  const double *l, *ssq;  // [N]
  double lmax;
  double center[RSF_LAW_GRID_MAX_PARAMS];  // of (Dc, a, b)
};

// One workgroup per column c = i1 + n1 i2: fields[c][RSF_LAW_GRID_FIELDS], the sums over the column's nodes of W = ((w0 w1) w2) e,
// e = exp(l - lmax) (0 for l = -inf), times 1, dq_0 .. dq_2, dq_0 dq_0, dq_0 dq_1, dq_0 dq_2, dq_1 dq_1, dq_1 dq_2, dq_2 dq_2, SSq, SSq^2;
// dq = q - center with q re-formed from the index by law_grid_point.  Thread t takes nodes t, t + blockDim.x, ... in that order,
// then wave_sum, then the waves in index order (block_fields_store).
template <int D>
__global__ void __launch_bounds__(kMaxBlock) law_grid_moments_kernel(LawMomentArgs A, double *__restrict__ fields) {
  __shared__ double sh[kMaxBlock / 64][RSF_LAW_GRID_FIELDS];
  const int64_t c = blockIdx.x, base = c * A.G.n[0];
  double s[RSF_LAW_GRID_FIELDS];
#pragma unroll
  for (int f = 0; f < RSF_LAW_GRID_FIELDS; ++f) s[f] = 0.0;
  for (int t = threadIdx.x; t < A.G.n[0]; t += blockDim.x) {
    double q[3] = {A.center[0], A.center[1], A.center[2]};
    uint32_t iz[3];
    law_grid_point<D>(A.G, A.M, (uint32_t)(base + t), q, iz);
    const double v = A.l[base + t];
    const bool fin = __builtin_isfinite(v);
    const double e = fin ? exp(v - A.lmax) : 0.0;
    const double W = ((A.G.w[0][iz[0]] * A.G.w[1][iz[1]]) * A.G.w[2][iz[2]]) * e, sq = fin ? A.ssq[base + t] : 0.0;
    double dq[3], wd[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) { dq[p] = q[p] - A.center[p]; wd[p] = W * dq[p]; }
    const double wq = W * sq;
    s[0] += W;
    int f = 4;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      s[1 + p] += wd[p];
#pragma unroll
      for (int r = p; r < 3; ++r, ++f) s[f] = __builtin_fma(wd[p], dq[r], s[f]);
    }
    s[10] += wq;
    s[11] = __builtin_fma(wq, sq, s[11]);
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int f = 0; f < RSF_LAW_GRID_FIELDS; ++f) {
    const double v = wave_sum(s[f]);
    if ((threadIdx.x & 63) == 0) sh[wave][f] = v;
  }
  __syncthreads();
  block_fields_store(sh, RSF_LAW_GRID_FIELDS, fields, c * RSF_LAW_GRID_FIELDS);
}

}  // namespace rsfk
