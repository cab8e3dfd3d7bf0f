// rsf_predict.h — posterior predictive checks of pooled draws (include/rsf_predict.h), the kernels:
//   predict_kernel         one lane per draw: the float64 RK4 tier code driven by rsf::integrate_lockstep, and at every
//                          completed output sample the wave's 64 values y_ik go through an LDS tile to the lanes that reduce them;
//   predict_select_kernel  exact order statistics of every row of a materialised series by rank_select, then rank_lerp.
// The per-wave partials are summed in index order by rsfh::sum_in_order (rsf_host.h), in two levels: slabs of kPredSlab waves,
// then the slabs.  No float atomics; every sum across lanes, waves and workgroups has a fixed order, so the same draws give the same bits.
//
// The per-sample hook.  A wave parks its 64 samples of an output time in one slot of a ring of kPredSlots slots (64 doubles
// each) — a conflict-free store, lane = bank.  Once a trip of RK4 steps is done and at least kPredTile slots are filled, the
// wave reads them back transposed: lane l = 8 g + m owns output time (tile's first + g) and the eight draws m + 8 ((t + g) & 7),
// t = 0..7 — rotated by g so that the 64 lanes of one read hit 64 different doubles.  Each lane evaluates l, exp and erfc for its
// eight draws with the draws' constants (read from LDS, written once per launch), accumulates the seven sums privately, and
// three DPP butterfly steps (quad_perm x2, row_half_mirror) leave the totals of the eight lanes in all of them; lane 8 g + f
// then stores field f of time g: one 512-byte row store per tile.  Per output sample that is one element evaluation per lane
// and 21/8 DPP pairs per field set, instead of six full-wave reductions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rsf_kernel_common.h"
#include "rsf_device.h"
#include "rsf_rank_device.h"
#include "rsf_predict_hook.h"

namespace rsfk {

template <int D, bool DAMP, bool WANT_SERIES>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) predict_kernel(Consts K, PredictArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  static_assert(rsf::kLockstepTrip <= kPredSlots - (kPredTile - 1), "a trip's samples fit the ring behind the left-over ones");
  const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + t;
  const int64_t wave_first = i - lane;
  const bool active = i < A.n;
  const int nvalid = (int)(A.n - wave_first < 64 ? (A.n - wave_first > 0 ? A.n - wave_first : 0) : 64);
  double *ring = lds + A.tab_doubles + wave * kPredWaveDoubles, *par = ring + kPredSlots * 64;
  double *wave_part = A.part + ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * (int64_t)K.nout * kPredFields;
  double pq[3] = {1000.0, K.a_def, K.b_def};  // lanes past the last draw carry a harmless Dc
  double s2 = 1.0;
  if (active) {
    pq[0] = A.q[i * D];
    if (D == 3) { pq[1] = A.q[i * D + 1]; pq[2] = A.q[i * D + 2]; }
    s2 = A.std2[i];
  }
  par[lane] = -0.5 * log(6.283185307179586476925 * s2);
  par[64 + lane] = 0.5 / s2;
  par[128 + lane] = 1.0 / sqrt(2.0 * s2);
  par[192 + lane] = s2;
  const rsf::Lane L = rsf::make_lane<DAMP>(pq[0], pq[1], pq[2], K);
  rsf::State st = rsf::initial_state(pq[0], L, K);
  // ring of parked samples: `cnt` filled slots from `head`, the first of them output time `kt` (all wave-uniform)
  int head = 0, cnt = 0, kt = 0, kabs = 0;
  auto park = [&](double y) {
    ring[((head + cnt) & (kPredSlots - 1)) * 64 + lane] = y;
    if (WANT_SERIES && active) A.series[(int64_t)kabs * A.n + i] = y;
    ++cnt;
    ++kabs;
  };
  auto flush = [&](int count) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    predict_flush(ring, par, A, K.nout, head, count, kt, nvalid, wave_part);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    head = (head + count) & (kPredSlots - 1);
    cnt -= count;
    kt += count;
  };
  park(0.0);  // y_i0 = 0
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    rsf::stage_chunk(lds, K, k0, kn);
    rsf::integrate_lockstep<DAMP>(lds, K, L, st, kn, [&](double ak, int) { park(ak); }, [&] { if (cnt >= kPredTile) flush(kPredTile); });
  }
  while (cnt > 0) flush(cnt < kPredTile ? cnt : kPredTile);
}

// ---- exact quantiles of every row ---------------------------------------------------------------------------------------
constexpr int kPredSelectThreads = 256;
constexpr int kPredMaxRanks = 32;  // two order statistics per probability, RSF_PREDICT_MAX_PROBS = 16

struct PredictProbs {
  double p[kPredMaxRanks / 2];
};

// One workgroup per row of series[nout][n]: both order statistics of np.quantile's "linear" method per probability by
// rank_select on rank_key's order-preserving map (rsf_diag_rank.h), then rank_lerp.
__global__ void __launch_bounds__(kPredSelectThreads)
predict_select_kernel(int64_t n, int64_t nout, const double *__restrict__ series, int nprobs, PredictProbs P, double *__restrict__ out) {
  __shared__ RankSelect<kPredMaxRanks> sel;
  __shared__ uint32_t nonfinite;
  const int nr = 2 * nprobs;
  const int64_t k = blockIdx.x;
  const double *row = series + k * n;
  const unsigned t = threadIdx.x;
  int64_t lo, hi;
  double g;
  if (t < (unsigned)nr) {
    rank_pair(n, P.p[t >> 1], lo, hi, g);
    sel.want[t] = (uint32_t)((t & 1) ? hi : lo);
  }
  if (t == 0) nonfinite = 0;
  rank_select(sel, nr, n, [&](int64_t j, int pass) {
    const double v = row[j];
    if (pass == 0 && !isfinite(v)) nonfinite = 1;  // (every writer stores the same value; read behind the select's last barrier)
    return rank_key(v);
  });
  if (t < (unsigned)nprobs) {
    rank_pair(n, P.p[t], lo, hi, g);
    const double v = rank_lerp(rank_value(sel.prefix[2 * t]), rank_value(sel.prefix[2 * t + 1]), g);
    out[(int64_t)t * nout + k] = nonfinite ? __longlong_as_double(0x7ff8000000000000ll) : v;
  }
}

}  // namespace rsfk
