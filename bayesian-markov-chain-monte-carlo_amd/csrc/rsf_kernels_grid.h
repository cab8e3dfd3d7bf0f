// rsf_kernels_grid.h — the exact posterior on a tensor quadrature grid (include/rsf_grid.h): grid_logtarget_kernel,
// grid_max_kernel, grid_max_finish_kernel, grid_columns_kernel, grid_m0_kernel, grid_cum0_kernel, grid_draw_kernel,
// grid_cdf_kernel.  Included by rsf_grid.hip only.
//
// Reproducibility: every sum below has an order fixed by the shape of the grid — per thread in node order, per wave by the
// shuffle tree, the waves of a workgroup and the columns in index order.  No floating-point atomic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_grid.h"
#include "rsf_kernel_common.h"
#include "rsf_device.h"

namespace rsfk {

constexpr int kGridBlocks = 1024;     // workgroups of grid_max_kernel at most: four per CU
constexpr int kGridHead = 4;          // largest finite l, finite entries, -inf entries, unused
// Register budget of grid_logtarget_kernel: three workgroups per CU, i.e. three waves per SIMD (at most 168 registers), the occupancy
// of evidence_logtarget_kernel<3, *>.  With kMinBlocks (2) the compiler took 170 to 172 for the undamped instantiations; held to
// 168 they compile without scratch — but for undamped PRODUCT, which then spills two registers around the full tier's loop: that one
// keeps kMinBlocks, 172 registers and no scratch (profiles/grid/resource_report.txt)
constexpr int grid_min_blocks(bool damp, int coord) { return (!damp && coord == RSF_GRID_PRODUCT) ? kMinBlocks : 3; }
constexpr uint32_t kGridSlotU2 = 3;   // Philox slot of the third uniform, as rsf_smc_init's (rsf_kernels_smc.h)

// the grid of one call: a kernel argument, so that every entry is a scalar register.  x and w point at device copies of the axes;
// an axis the grid lacks has n = 1 and one node 0 of weight 1
struct GridAxes {
  int32_t n[RSF_GRID_MAX_PARAMS];
  const double *x[RSF_GRID_MAX_PARAMS], *w[RSF_GRID_MAX_PARAMS];
};

// ---- the fused hot path -------------------------------------------------------------------------------------------------
struct GridTargetArgs {
  int64_t N;
  GridAxes G;
  double *l, *ssq;  // [N]
  double shape;
  double lo[RSF_GRID_MAX_PARAMS], hi[RSF_GRID_MAX_PARAMS];
};

// evidence_logtarget_kernel's arrangement (rsf_kernels_evidence.h) with the point formed from the flat index: one lane per node, a
// wave holds 64 consecutive axis-0 nodes.  A lane outside the CLOSED box, or past the last node, rides along with a harmless
// point; a WAVE without a lane inside skips the solve (it still takes part in the staging, whose barriers are the workgroup's).
template <int D, bool DAMP, int COORD>
__global__ void __launch_bounds__(kMaxBlock, grid_min_blocks(DAMP, COORD)) grid_logtarget_kernel(Consts K, GridTargetArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < A.N;
  double th[D], x1 = 1.0;
  if constexpr (D == 1) {
    th[0] = active ? A.G.x[0][i] : 0.5 * (A.lo[0] + A.hi[0]);
  } else {
    const uint32_t n0 = (uint32_t)A.G.n[0], n1 = (uint32_t)A.G.n[1];
    const uint32_t ii = active ? (uint32_t)i : 0u, r = ii / n0, i0 = ii - r * n0, i2 = r / n1, i1 = r - i2 * n1;
    const double x0 = A.G.x[0][i0];
    x1 = A.G.x[1][i1];
    th[0] = COORD == RSF_GRID_PRODUCT ? x0 / x1 : x0;
    th[1] = x1;
    th[2] = A.G.x[2][i2];
  }
  bool inb = active;
#pragma unroll
  for (int p = 0; p < D; ++p) inb = inb && (th[p] >= A.lo[p]) && (th[p] <= A.hi[p]);  // closed: a node on a face carries a weight
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
    const double jac = (COORD == RSF_GRID_PRODUCT && inb) ? -log(x1) : 0.0;
    A.l[i] = ok ? __builtin_fma(-A.shape, log(ssq), jac) : -INFINITY;
    A.ssq[i] = inb ? ssq : __longlong_as_double(0x7ff8000000000000ll);
  }
}

// ---- lmax: a pass of its own ------------------------------------------------------------------------------------------------
// part[block][kGridHead] = [largest finite l (-inf: none), finite entries, -inf entries, 0]; NaN and +inf are in neither count
__global__ void __launch_bounds__(kMaxBlock) grid_max_kernel(int64_t n, const double *__restrict__ l, double *__restrict__ part) {
  __shared__ double sh[kMaxBlock / 64][kGridHead];
  double m = -INFINITY, nf = 0.0, ni = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = l[i];
    const bool fin = __builtin_isfinite(v);
    m = fin ? fmax(m, v) : m;
    nf += fin ? 1.0 : 0.0;
    ni += v == -INFINITY ? 1.0 : 0.0;
  }
  m = wave_all_ascending<true>(m);
  nf = wave_sum(nf);
  ni = wave_sum(ni);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[wave][0] = m; sh[wave][1] = nf; sh[wave][2] = ni; sh[wave][3] = 0.0; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (unsigned w = 1; w < blockDim.x / 64; ++w) { sh[0][0] = fmax(sh[0][0], sh[w][0]); sh[0][1] += sh[w][1]; sh[0][2] += sh[w][2]; }
    for (int f = 0; f < kGridHead; ++f) part[(int64_t)blockIdx.x * kGridHead + f] = sh[0][f];
  }
}

// one thread: the head of all blocks (the maximum is order-free, the counts are exact integers)
__global__ void __launch_bounds__(64) grid_max_finish_kernel(int nblocks, const double *__restrict__ part, double *__restrict__ head) {
  if (threadIdx.x != 0) return;
  double m = -INFINITY, nf = 0.0, ni = 0.0;
  for (int b = 0; b < nblocks; ++b) { m = fmax(m, part[b * kGridHead]); nf += part[b * kGridHead + 1]; ni += part[b * kGridHead + 2]; }
  head[0] = m; head[1] = nf; head[2] = ni; head[3] = 0.0;
}

// ---- the reductions -----------------------------------------------------------------------------------------------------------
struct GridColArgs {
  GridAxes G;
  int64_t ncol;
  const double *l, *ssq;  // [N]
  double lmax, center;
};

// e = exp(l - lmax), 0 for l = -inf (and for every l when nothing is finite: lmax = -inf)
__device__ __forceinline__ double grid_e(double l, double lmax) { return __builtin_isfinite(l) ? exp(l - lmax) : 0.0; }

// One workgroup per column: fields[c][RSF_GRID_FIELDS].  Thread t takes nodes t, t + blockDim.x, ... in that order, then wave_sum,
// then the waves in index order (block_fields_store).
__global__ void __launch_bounds__(kMaxBlock) grid_columns_kernel(GridColArgs A, double *__restrict__ fields) {
  __shared__ double sh[kMaxBlock / 64][RSF_GRID_FIELDS];
  const int64_t c = blockIdx.x, base = c * A.G.n[0];
  double s[RSF_GRID_FIELDS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < A.G.n[0]; t += blockDim.x) {
    const double v = A.l[base + t];
    const bool fin = __builtin_isfinite(v);
    const double we = A.G.w[0][t] * grid_e(v, A.lmax), dx = A.G.x[0][t] - A.center, q = fin ? A.ssq[base + t] : 0.0;
    const double wd = we * dx, wq = we * q;
    s[0] += we;
    s[1] += wd;
    s[2] = __builtin_fma(wd, dx, s[2]);
    s[3] += wq;
    s[4] = __builtin_fma(wq, q, s[4]);
    s[5] += v == -INFINITY ? 1.0 : 0.0;
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int f = 0; f < RSF_GRID_FIELDS; ++f) {
    const double v = wave_sum(s[f]);
    if ((threadIdx.x & 63) == 0) sh[wave][f] = v;
  }
  __syncthreads();
  block_fields_store(sh, RSF_GRID_FIELDS, fields, c * RSF_GRID_FIELDS);
}

// the axis-0 marginal: one thread per i0, the columns in index order
__global__ void __launch_bounds__(kMaxBlock) grid_m0_kernel(GridColArgs A, double *__restrict__ m0) {
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 >= A.G.n[0]) return;
  double s = 0.0;
  int64_t at = i0;
  for (int i2 = 0; i2 < A.G.n[2]; ++i2)
    for (int i1 = 0; i1 < A.G.n[1]; ++i1, at += A.G.n[0]) s = __builtin_fma(A.G.w[1][i1] * A.G.w[2][i2], grid_e(A.l[at], A.lmax), s);
  m0[i0] = s;
}

// the trapezoid CDF along axis 0, one thread per column: the cells added in node order, then the division by the last entry
__global__ void __launch_bounds__(64) grid_cum0_kernel(GridColArgs A, double *__restrict__ cum0) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.ncol) return;
  const int n0 = A.G.n[0];
  const int64_t base = c * n0;
  double F = 0.0, ep = grid_e(A.l[base], A.lmax), xp = A.G.x[0][0];
  cum0[base] = 0.0;
  for (int k = 1; k < n0; ++k) {
    const double e = grid_e(A.l[base + k], A.lmax), xk = A.G.x[0][k];
    F += 0.5 * (ep + e) * (xk - xp);
    cum0[base + k] = F;
    ep = e; xp = xk;
  }
  if (F > 0.0)
    for (int k = 1; k < n0; ++k) cum0[base + k] = cum0[base + k] / F;
}

// ---- draws and the CDF of q0 ----------------------------------------------------------------------------------------------------
// k = the largest index <= n - 2 with F[k] <= u (F[0] = 0 <= u); F has the stride 1
__device__ __forceinline__ int grid_cell(const double *__restrict__ F, int n, double u) {
  int lo = 0, hi = n - 2;  // invariant: F[lo] <= u
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (F[mid] <= u) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// x = x[k] + (u - F[k]) / (F[k+1] - F[k]) (x[k+1] - x[k]); x[k] where the cell has no mass.  node: the nearest node, a tie to the lower
__device__ __forceinline__ double grid_invert(const double *__restrict__ F, const double *__restrict__ x, int n, double u, int &k, int &node) {
  k = grid_cell(F, n, u);
  const double dF = F[k + 1] - F[k], dx = x[k + 1] - x[k];
  const double v = dF > 0.0 ? x[k] + (u - F[k]) / dF * dx : x[k];
  node = (v - x[k] <= x[k + 1] - v) ? k : k + 1;
  return v;
}

struct GridDrawArgs {
  GridAxes G;
  int64_t nd, offset;
  uint64_t seed;
  const double *cum0, *cum1, *cum2;  // [N], [n2][n1], [n2]
  double *q;                         // [nd][D]
  int32_t *cell;                     // [nd][D] or NULL
};

template <int D, int COORD>
__global__ void __launch_bounds__(kMaxBlock) grid_draw_kernel(GridDrawArgs A) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.nd) return;
  uint32_t w[4];
  double u[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
  rsf::draw_words(A.seed, (uint64_t)(A.offset + j), 0u, rsf::SLOT_U, w);
  u[0] = rsf::u53(w[0], w[1]);
  u[1] = rsf::u53(w[2], w[3]);
  if (D > 2) { rsf::draw_words(A.seed, (uint64_t)(A.offset + j), 0u, kGridSlotU2, w); u[2] = rsf::u53(w[0], w[1]); }
  int k[3] = {0, 0, 0}, i1 = 0, i2 = 0, i0;
  if (D > 2) v[2] = grid_invert(A.cum2, A.G.x[2], A.G.n[2], u[2], k[2], i2);
  if (D > 1) v[1] = grid_invert(A.cum1 + (int64_t)i2 * A.G.n[1], A.G.x[1], A.G.n[1], u[1], k[1], i1);
  v[0] = grid_invert(A.cum0 + ((int64_t)i2 * A.G.n[1] + i1) * A.G.n[0], A.G.x[0], A.G.n[0], u[0], k[0], i0);
  if (COORD == RSF_GRID_PRODUCT) v[0] = v[0] / v[1];
#pragma unroll
  for (int p = 0; p < D; ++p) {
    A.q[j * D + p] = v[p];
    if (A.cell) A.cell[j * D + p] = k[p];
  }
}

// F(xs_k) = sum over the columns in index order of pair[c] F0(xs_k [x1] | c), one thread per point
template <int COORD>
__global__ void __launch_bounds__(kMaxBlock)
grid_cdf_kernel(GridAxes G, const double *__restrict__ cum0, const double *__restrict__ pair, int64_t nx, const double *__restrict__ xs, double *__restrict__ F) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nx) return;
  const int n0 = G.n[0];
  const double *x0 = G.x[0];
  const double xq = xs[j];
  double s = 0.0;
  int64_t c = 0;
  for (int i2 = 0; i2 < G.n[2]; ++i2)
    for (int i1 = 0; i1 < G.n[1]; ++i1, ++c) {
      const double t = COORD == RSF_GRID_PRODUCT ? xq * G.x[1][i1] : xq;
      const double *Fc = cum0 + c * n0;
      double f;
      if (!(t > x0[0])) f = 0.0;
      else if (!(t < x0[n0 - 1])) f = 1.0;
      else {
        int lo = 0, hi = n0 - 2;  // the cell with x0[lo] <= t < x0[lo + 1]
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (x0[mid] <= t) lo = mid; else hi = mid - 1;
        }
        f = Fc[lo] + (t - x0[lo]) / (x0[lo + 1] - x0[lo]) * (Fc[lo + 1] - Fc[lo]);
      }
      s = __builtin_fma(pair[c], f, s);
    }
  F[j] = s;
}

}  // namespace rsfk
