// rsf_kernels_law_predict.h — the posterior predictive checks under a state law (include/rsf_law_predict.h), the kernels:
//   law_predict_kernel      one lane per draw: law_observe_kernel's solve, and at every output sample the wave's 64 values y_ik
//                           go through the LDS ring of rsf_predict_hook.h to the lanes that reduce them (predict_kernel's hook);
//   series_partials_kernel  the same reduction of a series that already exists: a wave owns the same 64 draws, loads a tile of
//                           output times into the same ring layout and calls the same predict_flush.
// Both write the per-wave fields [waves][nout][kPredFields], which the host sums in index order in rsf_predict_partials' two
// levels.  A tile is the kPredTile output times from a multiple of kPredTile in every kernel of the family, so a time has the same
// place in its tile, predict_flush adds its draws in the same order, and equal series give equal partials bit for bit, whichever
// kernel made them.  The step is rsf_kernels_law.h's law_step, the sample rsf_kernels_observe.h's observe_sample, the hook
// rsf_predict_hook.h's predict_flush: none of them restated.  Included by rsf_law_predict.hip only (series_partials_kernel is no
// template).  No atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_law_predict.h"
#include "rsf_kernels_observe.h"
#include "rsf_predict_hook.h"

namespace rsfk {

// The solve is law_observe_kernel's, call for call, in law_dr_solve's restatement (rsf_kernels_law_dr.h): make_lane,
// initial_state, law_step, the per-lane `scale` and the `first` sample — those two expressions written out here as there, because
// as functions shared with law_observe_kernel they change that kernel's instructions — and observe_sample with the observable a
// wave-uniform kernel argument.  No residual is wanted: the observation is not staged with the table (K.data is NULL), and
// observe_sample's residual against 0 is dead code.  A lane past n rides along with the harmless point (1000, a_def, b_def) and
// is excluded by nvalid; a wave wholly past n rides along too, so it takes stage_chunk's barriers and writes its (zero) rows
// like any other.  No tier, no guard: a NaN trajectory runs to its end, and predict_flush counts its samples.
// The ring never holds more than kPredTile samples here: a sample is parked per K.S steps and the tile flushed as soon as it is full.
template <int D, int LAW, bool DAMP, bool WANT_SERIES>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) law_predict_kernel(Consts K, PredictArgs A, int32_t observable) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + t;
  const int64_t wave_first = i - lane;
  const bool active = i < A.n;
  const int nvalid = (int)(A.n - wave_first < 64 ? (A.n - wave_first > 0 ? A.n - wave_first : 0) : 64);
  double *ring = lds + A.tab_doubles + wave * kPredWaveDoubles, *par = ring + kPredSlots * 64;
  double *wave_part = A.part + ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * (int64_t)K.nout * kPredFields;
  double pq[3] = {1000.0, K.a_def, K.b_def};
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
  const rsf::State s0 = rsf::initial_state(pq[0], L, K);
  double ms = s0.ms, x = s0.x, V = s0.V, vprev = s0.V;
  const double scale = observable == RSF_OBS_THETA ? pq[0] * K.inv_vref : L.kprime;
  const double first = observable == RSF_OBS_ACC ? 0.0 : observable == RSF_OBS_VELOCITY ? s0.V : observable == RSF_OBS_MU ? scale * s0.ms : s0.x * scale;
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
  park(first);
  int phase = 0;  // RK4 steps since the last output sample (wave-uniform)
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    rsf::stage_chunk(lds, K, k0, kn);
    const int nsteps = K.S * kn;
    for (int r = 0; r < nsteps; ++r) {
      const double *v = lds + 2 * r;
      V = __builtin_fma(L.h6v, law_step<LAW, DAMP>(ms, x, v[0], v[1], v[2], L, K), V);
      if (++phase == K.S) {
        phase = 0;
        double s, res;
        observe_sample(observable, V, vprev, ms, x, scale, 0.0, K, s, res);
        park(s);
        if (cnt >= kPredTile) flush(kPredTile);
      }
    }
  }
  if (cnt > 0) flush(cnt);
}

// The partials of a materialised series [nout][n]: law_predict_kernel's assignment of draws to waves, its LDS area per wave (no
// table in front: A.tab_doubles is 0) and its tiles.  Memory-bound: every element is read once, a tile's up to kPredTile loads of a
// lane in flight together, each a coalesced 512-byte row of the wave.
__global__ void __launch_bounds__(kMaxBlock) series_partials_kernel(PredictArgs A, int32_t nout) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + t;
  const int64_t wave_first = i - lane;
  const bool active = i < A.n;
  const int nvalid = (int)(A.n - wave_first < 64 ? (A.n - wave_first > 0 ? A.n - wave_first : 0) : 64);
  double *ring = lds + A.tab_doubles + wave * kPredWaveDoubles, *par = ring + kPredSlots * 64;
  double *wave_part = A.part + ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * (int64_t)nout * kPredFields;
  const double s2 = active ? A.std2[i] : 1.0;
  par[lane] = -0.5 * log(6.283185307179586476925 * s2);
  par[64 + lane] = 0.5 / s2;
  par[128 + lane] = 1.0 / sqrt(2.0 * s2);
  par[192 + lane] = s2;
  const double *col = A.series + (active ? i : 0);
  for (int k0 = 0; k0 < nout; k0 += kPredTile) {
    const int count = min(kPredTile, nout - k0);
    double y[kPredTile];
#pragma unroll
    for (int g = 0; g < kPredTile; ++g) y[g] = (active && g < count) ? col[(int64_t)(k0 + g) * A.n] : 0.0;
#pragma unroll
    for (int g = 0; g < kPredTile; ++g) ring[g * 64 + lane] = y[g];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    predict_flush(ring, par, A, nout, 0, count, k0, nvalid, wave_part);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace rsfk
