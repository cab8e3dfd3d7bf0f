// rsf_predict_hook.h — the per-sample hook of the predictive kernels: the constants of the wave's LDS area, PredictArgs, and
// predict_flush, which reduces a tile of parked output samples and stores the per-wave fields.  It defines no kernel, so every
// unit whose kernels reduce a series to the predictive partials includes it: rsf_predict.h (predict_kernel, whose header comment
// describes the hook) and rsf_kernels_law_predict.h (law_predict_kernel, series_partials_kernel).  One definition: equal
// samples give equal per-wave fields bit for bit, whichever kernel parked them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsf_kernel_common.h"
#include "rsf_device.h"

namespace rsfk {

constexpr int kPredFields = 8;   // per (wave, output time) in the workspace: the seven of RSF_PREDICT_FIELDS + sum of sigma^2
constexpr int kPredTile = 8;     // output times reduced per flush: 8 times x 8 lanes
constexpr int kPredSlots = 16;   // ring of parked samples: up to kPredTile - 1 left over + one trip's worth (<= 8)
constexpr int kPredParams = 4;   // per draw in LDS: -1/2 log(2 pi s2), 1/(2 s2), 1/sqrt(2 s2), s2
constexpr int kPredWaveDoubles = kPredSlots * 64 + kPredParams * 64;  // 10 KiB per wave
// LDS of a predict launch: the loading table chunk, then kPredWaveDoubles per wave.  Two workgroups of four waves per CU
// (160 KiB): 40 KiB of wave areas + at most this much table; nsteps 2000 (32 KB of loading values) stays resident.
constexpr size_t kPredTableBudget = 38 * 1024;
constexpr int kPredSlab = 64;    // waves per slab of the first level of the partials' sum

struct PredictArgs {
  int64_t n;
  const double *q;     // [n][D], the C ABI's layout
  const double *std2;  // [n]
  const double *data, *cy, *cl;  // [nout]
  double *part;        // [waves][nout][kPredFields]
  double *series;      // WANT_SERIES: [nout][n]
  int32_t tab_doubles; // offset of the wave areas behind the table chunk
};

// the sum over an aligned group of eight lanes, in all eight (a + b == b + a bit for bit, so the butterfly agrees everywhere)
__device__ __forceinline__ double pred_sum8(double v) {
  v += rsf::dpp_move<0xB1>(v);   // quad_perm [1,0,3,2]
  v += rsf::dpp_move<0x4E>(v);   // quad_perm [2,3,0,1]
  v += rsf::dpp_move<0x141>(v);  // row_half_mirror: the other quad of the eight
  return v;
}

// Reduces `count` (<= kPredTile) parked output times starting at ring slot `head`, absolute time k0, and stores their fields.
__device__ __forceinline__ void predict_flush(const double *ring, const double *par, const PredictArgs &A, int nout, int head, int count, int k0,
                                              int nvalid, double *wave_part) {
  const unsigned lane = threadIdx.x & 63;
  const int g = (int)(lane >> 3), m = (int)(lane & 7);
  const bool mine = g < count;
  const int k = mine ? k0 + g : k0;
  const double obs = A.data[k], cy = A.cy[k], cl = A.cl[k];
  const double *row = ring + ((head + g) & (kPredSlots - 1)) * 64;
  double s[kPredFields];
#pragma unroll
  for (int f = 0; f < kPredFields; ++f) s[f] = 0.0;
#pragma unroll 1
  for (int t = 0; t < 8; ++t) {
    const int i = m + 8 * ((t + g) & 7);
    const double y = row[i];
    const double lognorm = par[i], h = par[64 + i], isr = par[128 + i], s2 = par[192 + i];
    const bool valid = i < nvalid, use = valid && isfinite(y);
    const double ys = use ? y : cy;
    const double dy = ys - cy, r = obs - ys;
    const double dl = (lognorm - (r * r) * h) - cl;
    const double e = exp(dl), phi = 0.5 * erfc(-(r * isr));
    s[0] += use ? dy : 0.0;
    s[1] += use ? dy * dy : 0.0;
    s[2] += use ? dl : 0.0;
    s[3] += use ? dl * dl : 0.0;
    s[4] += use ? e : 0.0;
    s[5] += use ? phi : 0.0;
    s[6] += (valid && !use) ? 1.0 : 0.0;
    s[7] += valid ? s2 : 0.0;
  }
  double out = 0.0;
#pragma unroll
  for (int f = 0; f < kPredFields; ++f) {
    const double tot = pred_sum8(s[f]);
    out = m == f ? tot : out;
  }
  if (mine) wave_part[(int64_t)k * kPredFields + m] = out;
}

}  // namespace rsfk
