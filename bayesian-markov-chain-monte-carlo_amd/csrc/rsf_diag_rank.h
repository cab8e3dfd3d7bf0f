// rsf_diag_rank.h — rank-normalised diagnostics and order statistics of a kept trace x[n][C][d] (include/rsf_diag.h,
// rsf_diag_rank_*): a device sort of every parameter's n*C draws and the four derived series that the existing diagnostics
// kernels (rsf_diag.h) then reduce.  Included by rsf_diag.hip only, which holds the host orchestration; the device functions that
// the predictive kernels use as well (rank_ndtri among them) are in rsf_rank_device.h.
//
// Sort.  A draw becomes an order-preserving uint64 key (-0.0 folded onto +0.0) paired with its 32-bit flat index i*C + c, and the
// pairs go through an LSD radix sort, 8 bits per pass:
//   rank_key_kernel       keys and indices, per workgroup the digit histograms of all 8 passes at once and a non-finite count;
//   rank_hist_kernel      their fixed-order sum.  The host reads it and skips every pass in which one bucket holds every key
//                         (sign and exponent bytes, mostly).
//   rank_upsweep_kernel   per tile of kTile keys: its 256-bucket histogram, bucket-major [bucket][tile].
//   rank_offsets_kernel   one workgroup per bucket: exclusive scan over the tiles, in tile order, plus the bucket's start.
//   rank_scatter_kernel   stable: ranks each key among the tile's keys of its bucket (wave match on the digit's 8 bits, then the
//                         waves in order), reorders the tile in LDS by bucket and writes each bucket's run contiguously.
// Ranks.  On the sorted pairs, with f = 1 for a split-set draw (row != the middle row of an odd n):
//   rank_tile_kernel      per tile: sum f, last run head, first run head (a head is a key that differs from its predecessor);
//   rank_carry_kernel     one workgroup, fixed order: exclusive sum of f over tiles, the last head before and the first head after
//                         each tile;
//   rank_prefix_kernel    P[j] = sum of f over sorted positions < j, P[A] = T;
//   rank_z_kernel         per position: its run [start, next head) by a max-scan and a min-scan with the tile carries, L = P[start],
//                         L + E = P[next head], r = L + (E + 1)/2, z = ndtri((r - 3/8) / (T + 1/4)), written to the draw's place
//                         (0 for the middle row).
// Order statistics (rank_order_kernel: median, np.quantile "linear" with NumPy's _lerp; rank_hdi_* : the first index of the
// narrowest window), the tail indicators (rank_indicator_kernel) and the per-series range (rank_range_*) complete it.  Every
// reduction is in a fixed order or is order-independent (integer counts, lexicographic min, min/max), so the same trace gives the
// same bits on every call; no float atomics, ScratchSize 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsf_rank_device.h"

namespace rsfk {

constexpr int kRankThreads = 256;                       // workgroup size of every rank kernel
constexpr int kRankItems = 16;                          // keys per thread and tile
constexpr int kRankTile = kRankThreads * kRankItems;    // keys per tile
constexpr int kRankDigits = 8;                          // 8 passes of 8 bits
constexpr int kRankKeyBlocks = 1024;                    // rank_key_kernel: grid-stride, so few histogram flushes
constexpr int kRankReduceBlocks = 1024;                 // HDI and range reductions: per-workgroup partials, then one workgroup
constexpr int kRankStatHead = 10;                       // RSF_DIAG_RANK_STATS
// stats[p][kRankStatHead + n_probs]: fields
constexpr int kStMedian = 0, kStQ05 = 1, kStQ95 = 2, kStHdiLo = 3, kStHdiHi = 4, kStNonFinite = 5, kStConst = 6;

// ---- workgroup primitives (blockDim.x = kRankThreads) ------------------------------------------
// lanes of the wave whose digit equals this lane's (0 for an invalid lane): one ballot per digit bit
__device__ __forceinline__ uint64_t rank_match(uint32_t dig, bool valid) {
  uint64_t peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (dig >> b) & 1u;
    const uint64_t m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  return valid ? peers : 0;
}

struct RankSum { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
struct RankMax { template <class T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct RankMin { template <class T> __device__ T operator()(T a, T b) const { return a < b ? a : b; } };

// exclusive scan over the workgroup's threads in thread order; *total = the reduction of every thread's v
template <class T, class Op>
__device__ T rank_block_scan(T v, T ident, Op op, T *sh /* [kRankThreads / 64] */, T *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T u = __shfl_up(inc, off, 64);
    if (lane >= off) inc = op(u, inc);
  }
  T exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = ident;
  __syncthreads();
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  T pre = ident, all = ident;
  for (int w = 0; w < kRankThreads / 64; ++w) {
    if (w == wave) pre = all;
    all = op(all, sh[w]);
  }
  *total = all;
  return op(pre, exc);
}

// the same over the threads after this one (a suffix scan): the scan of the mirrored thread order
template <class T, class Op>
__device__ T rank_block_rscan(T v, T ident, Op op, T *mirror /* [kRankThreads] */, T *sh, T *total) {
  __syncthreads();
  mirror[kRankThreads - 1 - threadIdx.x] = v;
  __syncthreads();
  const T m = mirror[threadIdx.x];
  const T e = rank_block_scan(m, ident, op, sh, total);
  __syncthreads();
  mirror[threadIdx.x] = e;
  __syncthreads();
  return mirror[kRankThreads - 1 - threadIdx.x];
}

// ---- sort ------------------------------------------------------------------------------------
// Keys and indices of parameter p's draws, value v = x (folded = false) or |x - m| (folded, m = stats median), and per workgroup
// the 8 digit histograms and a non-finite count: part[block][kRankHist].  A workgroup sweeps tiles grid-stride.
constexpr int kRankHist = kRankDigits * 256 + 1;
__global__ void __launch_bounds__(kRankThreads)
rank_key_kernel(int64_t A, int d, int p, const double *__restrict__ x, bool folded, const double *__restrict__ stats,
                uint64_t *__restrict__ keys, uint32_t *__restrict__ idx, uint32_t *__restrict__ part) {
  __shared__ uint32_t h[kRankDigits][256];
  for (int i = threadIdx.x; i < kRankDigits * 256; i += kRankThreads) (&h[0][0])[i] = 0;
  __syncthreads();
  const double m = folded ? stats[kStMedian] : 0.0;
  uint32_t bad = 0;
  for (int64_t base = (int64_t)blockIdx.x * kRankTile; base < A; base += (int64_t)gridDim.x * kRankTile) {
    for (int k = 0; k < kRankItems; ++k) {
      const int64_t j = base + (int64_t)k * kRankThreads + threadIdx.x;
      const bool valid = j < A;
      uint64_t key = 0;
      if (valid) {
        double v = x[j * d + p];
        bad |= !isfinite(v);
        if (folded) v = fabs(v - m);
        key = rank_key(v);
        keys[j] = key;
        idx[j] = (uint32_t)j;
      }
#pragma unroll
      for (int g = 0; g < kRankDigits; ++g) {
        const uint32_t dig = (uint32_t)(key >> (8 * g)) & 255u;
        const uint32_t first = __shfl(dig, 0, 64);
        if (__all(!valid || dig == first)) {  // the common case for the high bytes: one add for the wave
          const uint32_t cnt = (uint32_t)__popcll(__ballot(valid));
          if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&h[g][first], cnt);
        } else if (valid) {
          atomicAdd(&h[g][dig], 1u);
        }
      }
    }
  }
  __syncthreads();
  uint32_t *o = part + (int64_t)blockIdx.x * kRankHist;
  for (int i = threadIdx.x; i < kRankDigits * 256; i += kRankThreads) o[i] = (&h[0][0])[i];
  const uint32_t nbad = (uint32_t)__syncthreads_count(bad);
  if (threadIdx.x == 0) o[kRankDigits * 256] = nbad;
}

// hist[i] = sum over the key kernel's workgroups of part[b][i], in workgroup order
__global__ void __launch_bounds__(kRankThreads)
rank_hist_kernel(int nparts, const uint32_t *__restrict__ part, uint32_t *__restrict__ hist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kRankHist) return;
  uint32_t t = 0;
  for (int b = 0; b < nparts; ++b) t += part[(int64_t)b * kRankHist + i];
  hist[i] = t;
}

// per tile: its histogram of digit (key >> shift) & 255, stored bucket-major th[bucket][tile]
__global__ void __launch_bounds__(kRankThreads)
rank_upsweep_kernel(int64_t A, int shift, const uint64_t *__restrict__ keys, uint32_t *__restrict__ th, int64_t ntiles) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kRankTile;
  const int lane = threadIdx.x & 63;
#pragma unroll 4
  for (int k = 0; k < kRankItems; ++k) {
    const int64_t j = base + (int64_t)k * kRankThreads + threadIdx.x;
    const bool valid = j < A;
    const uint32_t dig = valid ? (uint32_t)(keys[j] >> shift) & 255u : 0u;
    const uint64_t peers = rank_match(dig, valid);
    if (valid && __ffsll((unsigned long long)peers) - 1 == lane) atomicAdd(&h[dig], (uint32_t)__popcll(peers));
  }
  __syncthreads();
  th[(int64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// workgroup b = bucket: th[b][t] <- start of bucket b + sum over tiles t' < t of th[b][t'] (in place), tile order
__global__ void __launch_bounds__(kRankThreads)
rank_offsets_kernel(const uint32_t *__restrict__ hist, uint32_t *__restrict__ th, int64_t ntiles) {
  __shared__ uint32_t sh[kRankThreads / 64];
  __shared__ uint32_t chunk[kRankTile];
  const int b = blockIdx.x;
  uint32_t start = 0;
  for (int i = 0; i < b; ++i) start += hist[i];
  uint32_t *row = th + (int64_t)b * ntiles;
  uint32_t carry = start;
  for (int64_t c0 = 0; c0 < ntiles; c0 += kRankTile) {
    const int64_t len = ntiles - c0 < kRankTile ? ntiles - c0 : kRankTile;
    __syncthreads();
    for (int i = threadIdx.x; i < kRankTile; i += kRankThreads) chunk[i] = i < len ? row[c0 + i] : 0u;
    __syncthreads();
    uint32_t v[kRankItems], s = 0;
#pragma unroll
    for (int k = 0; k < kRankItems; ++k) { v[k] = chunk[threadIdx.x * kRankItems + k]; s += v[k]; }
    uint32_t tot;
    uint32_t pre = carry + rank_block_scan(s, 0u, RankSum(), sh, &tot);
#pragma unroll
    for (int k = 0; k < kRankItems; ++k) { chunk[threadIdx.x * kRankItems + k] = pre; pre += v[k]; }
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += kRankThreads) row[c0 + i] = chunk[i];
    carry += tot;
  }
}

// stable scatter of one tile by digit (key >> shift) & 255, to off[bucket][tile] + the key's rank in the tile's bucket
__global__ void __launch_bounds__(kRankThreads)
rank_scatter_kernel(int64_t A, int shift, const uint64_t *__restrict__ kin, const uint32_t *__restrict__ iin,
                    uint64_t *__restrict__ kout, uint32_t *__restrict__ iout, const uint32_t *__restrict__ off, int64_t ntiles) {
  __shared__ uint64_t kbuf[kRankTile];
  __shared__ uint32_t ibuf[kRankTile];
  __shared__ uint32_t wcnt[kRankThreads / 64][256];
  __shared__ uint32_t cnt[256], tstart[256], goff[256];
  __shared__ uint32_t sh[kRankThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t base = (int64_t)blockIdx.x * kRankTile;
  goff[t] = off[(int64_t)t * ntiles + blockIdx.x];
  cnt[t] = 0;
#pragma unroll
  for (int w = 0; w < kRankThreads / 64; ++w) wcnt[w][t] = 0;
  __syncthreads();
  uint64_t kk[kRankItems];
  uint32_t ii[kRankItems], rk[kRankItems];
#pragma unroll
  for (int k = 0; k < kRankItems; ++k) {  // round k: tile positions k*256 + t, in thread order; rounds in order
    const int64_t j = base + (int64_t)k * kRankThreads + t;
    const bool valid = j < A;
    kk[k] = valid ? kin[j] : 0ull;
    ii[k] = valid ? iin[j] : 0u;
    const uint32_t dig = (uint32_t)(kk[k] >> shift) & 255u;
    const uint64_t peers = rank_match(dig, valid);
    const uint32_t below = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    if (valid && below == 0) wcnt[wave][dig] = (uint32_t)__popcll(peers);
    __syncthreads();
    uint32_t r = cnt[dig] + below;
    for (int w = 0; w < wave; ++w) r += wcnt[w][dig];
    rk[k] = r;
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kRankThreads / 64; ++w) { s += wcnt[w][t]; wcnt[w][t] = 0; }
    cnt[t] += s;
    __syncthreads();
  }
  uint32_t tot;
  tstart[t] = rank_block_scan(cnt[t], 0u, RankSum(), sh, &tot);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kRankItems; ++k) {
    const int64_t j = base + (int64_t)k * kRankThreads + t;
    if (j < A) {
      const uint32_t q = tstart[(uint32_t)(kk[k] >> shift) & 255u] + rk[k];
      kbuf[q] = kk[k];
      ibuf[q] = ii[k];
    }
  }
  __syncthreads();
  const int64_t len = A - base < kRankTile ? A - base : kRankTile;
#pragma unroll 4
  for (int k = 0; k < kRankItems; ++k) {
    const int q = k * kRankThreads + t;
    if (q < len) {
      const uint64_t key = kbuf[q];
      const uint32_t dig = (uint32_t)(key >> shift) & 255u;
      const int64_t o = (int64_t)goff[dig] + (q - (int64_t)tstart[dig]);
      kout[o] = key;
      iout[o] = ibuf[q];
    }
  }
}

// ---- ranks -----------------------------------------------------------------------------------
struct RankShape {
  int64_t A;               // draws n*C
  int64_t mid0, mid1;      // flat indices [mid0, mid1) of the middle row left out of the split set (n odd), else empty
  int d, p;                // parameters, this parameter
  double T;                // split-set size 2*C*N
  __device__ bool member(int64_t j) const { return j < mid0 || j >= mid1; }
};

// thread t of a tile holds sorted positions base + t*kRankItems + k
__device__ __forceinline__ void rank_load(const RankShape &s, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                                          int64_t base, uint64_t (&kk)[kRankItems], uint32_t (&ff)[kRankItems],
                                          bool (&head)[kRankItems], uint32_t *ii) {
  const int64_t j0 = base + (int64_t)threadIdx.x * kRankItems;
  uint64_t prev = j0 > 0 && j0 - 1 < s.A ? keys[j0 - 1] : 0ull;
#pragma unroll
  for (int k = 0; k < kRankItems; ++k) {
    const int64_t j = j0 + k;
    const bool valid = j < s.A;
    kk[k] = valid ? keys[j] : 0ull;
    const uint32_t ix = valid ? idx[j] : 0u;
    if (ii) ii[k] = ix;
    ff[k] = valid && s.member(ix);
    head[k] = valid && (j == 0 || kk[k] != prev);
    prev = kk[k];
  }
}

// per tile: sum f, last head position (0 if none), first head position (A if none)
__global__ void __launch_bounds__(kRankThreads)
rank_tile_kernel(RankShape s, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx, uint32_t *__restrict__ tm,
                 uint32_t *__restrict__ tlast, uint32_t *__restrict__ tfirst) {
  __shared__ uint32_t sh[kRankThreads / 64];
  const int64_t base = (int64_t)blockIdx.x * kRankTile, j0 = base + (int64_t)threadIdx.x * kRankItems;
  uint64_t kk[kRankItems];
  uint32_t ff[kRankItems];
  bool head[kRankItems];
  rank_load(s, keys, idx, base, kk, ff, head, nullptr);
  uint32_t m = 0, last = 0, first = (uint32_t)s.A;
#pragma unroll
  for (int k = 0; k < kRankItems; ++k) {
    m += ff[k];
    if (head[k]) { last = (uint32_t)(j0 + k); first = first < (uint32_t)(j0 + k) ? first : (uint32_t)(j0 + k); }
  }
  uint32_t a, b, c;
  (void)rank_block_scan(m, 0u, RankSum(), sh, &a);
  (void)rank_block_scan(last, 0u, RankMax(), sh, &b);
  (void)rank_block_scan(first, (uint32_t)s.A, RankMin(), sh, &c);
  if (threadIdx.x == 0) { tm[blockIdx.x] = a; tlast[blockIdx.x] = b; tfirst[blockIdx.x] = c; }
}

// one workgroup, in place: tm -> exclusive sum over earlier tiles, tlast -> last head before the tile (0), tfirst -> first head
// after the tile (A)
__global__ void __launch_bounds__(kRankThreads)
rank_carry_kernel(int64_t ntiles, uint32_t A, uint32_t *__restrict__ tm, uint32_t *__restrict__ tlast, uint32_t *__restrict__ tfirst) {
  __shared__ uint32_t sh[kRankThreads / 64];
  __shared__ uint32_t mirror[kRankThreads];
  uint32_t csum = 0, cmax = 0, cmin = A;
  for (int64_t c0 = 0; c0 < ntiles; c0 += kRankTile) {  // forward: sum and max
    const int64_t i0 = c0 + (int64_t)threadIdx.x * kRankItems;
    uint32_t vm[kRankItems], vl[kRankItems], sm = 0, sl = 0;
#pragma unroll
    for (int k = 0; k < kRankItems; ++k) {
      const bool ok = i0 + k < ntiles;
      vm[k] = ok ? tm[i0 + k] : 0u;
      vl[k] = ok ? tlast[i0 + k] : 0u;
      sm += vm[k];
      sl = sl > vl[k] ? sl : vl[k];
    }
    uint32_t tsum, tmax;
    uint32_t pm = csum + rank_block_scan(sm, 0u, RankSum(), sh, &tsum);
    uint32_t pl = rank_block_scan(sl, 0u, RankMax(), sh, &tmax);
    pl = pl > cmax ? pl : cmax;
#pragma unroll
    for (int k = 0; k < kRankItems; ++k) {
      if (i0 + k < ntiles) { tm[i0 + k] = pm; tlast[i0 + k] = pl; }
      pm += vm[k];
      pl = pl > vl[k] ? pl : vl[k];
    }
    csum += tsum;
    cmax = cmax > tmax ? cmax : tmax;
  }
  const int64_t nchunks = (ntiles + kRankTile - 1) / kRankTile;
  for (int64_t ch = nchunks - 1; ch >= 0; --ch) {  // backward: min
    const int64_t i0 = ch * kRankTile + (int64_t)threadIdx.x * kRankItems;
    uint32_t vf[kRankItems], sf = A;
#pragma unroll
    for (int k = 0; k < kRankItems; ++k) {
      vf[k] = i0 + k < ntiles ? tfirst[i0 + k] : A;
      sf = sf < vf[k] ? sf : vf[k];
    }
    uint32_t tmin;
    uint32_t pf = rank_block_rscan(sf, A, RankMin(), mirror, sh, &tmin);
    pf = pf < cmin ? pf : cmin;
#pragma unroll
    for (int k = kRankItems - 1; k >= 0; --k) {
      if (i0 + k < ntiles) tfirst[i0 + k] = pf;
      pf = pf < vf[k] ? pf : vf[k];
    }
    cmin = cmin < tmin ? cmin : tmin;
  }
}

// P[j] = split-set draws at sorted positions < j; P[A] = all of them
__global__ void __launch_bounds__(kRankThreads)
rank_prefix_kernel(RankShape s, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ tp,
                   uint32_t *__restrict__ P) {
  __shared__ uint32_t sh[kRankThreads / 64];
  const int64_t base = (int64_t)blockIdx.x * kRankTile, j0 = base + (int64_t)threadIdx.x * kRankItems;
  uint64_t kk[kRankItems];
  uint32_t ff[kRankItems];
  bool head[kRankItems];
  rank_load(s, keys, idx, base, kk, ff, head, nullptr);
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < kRankItems; ++k) m += ff[k];
  uint32_t tot;
  uint32_t pre = tp[blockIdx.x] + rank_block_scan(m, 0u, RankSum(), sh, &tot);
#pragma unroll
  for (int k = 0; k < kRankItems; ++k) {
    const int64_t j = j0 + k;
    if (j < s.A) P[j] = pre;
    pre += ff[k];
    if (j == s.A - 1) P[s.A] = pre;
  }
}

// z of every draw from its run [start, next head) among the sorted keys; out = series + p, stride d
__global__ void __launch_bounds__(kRankThreads)
rank_z_kernel(RankShape s, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ tlast,
              const uint32_t *__restrict__ tfirst, const uint32_t *__restrict__ P, double *__restrict__ out) {
  __shared__ uint32_t sh[kRankThreads / 64];
  __shared__ uint32_t mirror[kRankThreads];
  const int64_t base = (int64_t)blockIdx.x * kRankTile, j0 = base + (int64_t)threadIdx.x * kRankItems;
  const uint32_t A = (uint32_t)s.A;
  uint64_t kk[kRankItems];
  uint32_t ff[kRankItems], ii[kRankItems];
  bool head[kRankItems];
  rank_load(s, keys, idx, base, kk, ff, head, ii);
  uint32_t last = 0, first = A;
#pragma unroll
  for (int k = 0; k < kRankItems; ++k)
    if (head[k]) { last = (uint32_t)(j0 + k); first = first < (uint32_t)(j0 + k) ? first : (uint32_t)(j0 + k); }
  uint32_t tot;
  uint32_t start = rank_block_scan(last, 0u, RankMax(), sh, &tot);
  start = start > tlast[blockIdx.x] ? start : tlast[blockIdx.x];
  uint32_t next = rank_block_rscan(first, A, RankMin(), mirror, sh, &tot);
  next = next < tfirst[blockIdx.x] ? next : tfirst[blockIdx.x];
  uint32_t st[kRankItems];
#pragma unroll
  for (int k = 0; k < kRankItems; ++k) {
    if (head[k]) start = (uint32_t)(j0 + k);
    st[k] = start;
  }
  const double denom = s.T + 0.25;
#pragma unroll
  for (int k = kRankItems - 1; k >= 0; --k) {
    const int64_t j = j0 + k;
    if (j < s.A) {
      const uint32_t L = P[st[k]], LE = P[next];
      double z = 0.0;
      if (ff[k]) {
        const double r = 0.5 * (double)((uint64_t)LE + L + 1u);  // scipy rankdata "average": L + (E + 1) / 2
        z = rank_ndtri((r - 0.375) / denom);
      }
      if (ii[k] < A) out[(int64_t)ii[k] * s.d + s.p] = z;  // always true for a permutation; keeps a bad one in bounds
    }
    if (head[k]) next = (uint32_t)j;
  }
}

// ---- order statistics ------------------------------------------------------------------------
__device__ double rank_quantile(const uint64_t *__restrict__ s, int64_t A, double prob) {
  int64_t lo, hi;
  double g;
  rank_pair(A, prob, lo, hi, g);
  return rank_lerp(rank_value(s[lo]), rank_value(s[hi]), g);
}

// thread 0: median; 1, 2: quantiles 0.05, 0.95; 3 + i: probs[i]
__global__ void rank_order_kernel(const uint64_t *__restrict__ s, int64_t A, int nprobs, const double *__restrict__ probs,
                                  double *__restrict__ st) {
  for (int t = threadIdx.x; t < 3 + nprobs; t += blockDim.x) {
    if (t == 0)
      st[kStMedian] = A % 2 ? rank_value(s[(A - 1) / 2]) : (rank_value(s[A / 2 - 1]) + rank_value(s[A / 2])) / 2.0;
    else
      st[t == 1 ? kStQ05 : t == 2 ? kStQ95 : kRankStatHead + t - 3] = rank_quantile(s, A, t == 1 ? 0.05 : t == 2 ? 0.95 : probs[t - 3]);
  }
}

// I_lo = x <= q05, I_hi = x <= q95 for the split set (0 for the middle row); lo and hi = series 2 and 3, + p, stride d
__global__ void __launch_bounds__(kRankThreads)
rank_indicator_kernel(RankShape s, const double *__restrict__ x, const double *__restrict__ st, double *__restrict__ lo,
                      double *__restrict__ hi) {
  const double q05 = st[kStQ05], q95 = st[kStQ95];
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < s.A; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = j * s.d + s.p;
    const bool member = s.member(j);
    const double v = x[o];
    lo[o] = member && v <= q05 ? 1.0 : 0.0;
    hi[o] = member && v <= q95 ? 1.0 : 0.0;
  }
}

struct RankArg {  // (width, first index): the lexicographic minimum is the first index of the smallest width
  double w;
  int64_t i;
};
__device__ __forceinline__ RankArg rank_argmin(RankArg a, RankArg b) {
  return (b.w < a.w || (!(a.w < b.w) && b.i < a.i)) ? b : a;
}
__device__ RankArg rank_block_argmin(RankArg v, RankArg *sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    RankArg o;
    o.w = __shfl_down(v.w, off, 64);
    o.i = __shfl_down(v.i, off, 64);
    v = rank_argmin(v, o);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  RankArg r = sh[0];
  for (int w = 1; w < kRankThreads / 64; ++w) r = rank_argmin(r, sh[w]);
  return r;
}

// HDI: widths s[i + k] - s[i], i < A - k; per-workgroup (width, index) into part[block]
__global__ void __launch_bounds__(kRankThreads)
rank_hdi_kernel(const uint64_t *__restrict__ s, int64_t A, int64_t k, RankArg *__restrict__ part) {
  __shared__ RankArg sh[kRankThreads / 64];
  RankArg best{INFINITY, INT64_MAX};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A - k; i += (int64_t)gridDim.x * blockDim.x)
    best = rank_argmin(best, RankArg{rank_value(s[i + k]) - rank_value(s[i]), i});
  best = rank_block_argmin(best, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = best;
}

__global__ void __launch_bounds__(kRankThreads)
rank_hdi_final_kernel(const uint64_t *__restrict__ s, int64_t A, int64_t k, int nparts, const RankArg *__restrict__ part, double *__restrict__ st) {
  __shared__ RankArg sh[kRankThreads / 64];
  RankArg best{INFINITY, INT64_MAX};
  for (int b = threadIdx.x; b < nparts; b += blockDim.x) best = rank_argmin(best, part[b]);
  best = rank_block_argmin(best, sh);
  if (threadIdx.x == 0 && best.i >= 0 && best.i < A - k) {
    st[kStHdiLo] = rank_value(s[best.i]);
    st[kStHdiHi] = rank_value(s[best.i + k]);
  }
}

// range of series q (+ p, stride d) over the split set: per-workgroup (min, max) into part[block][2]
__global__ void __launch_bounds__(kRankThreads)
rank_range_kernel(RankShape s, const double *__restrict__ q, double *__restrict__ part) {
  __shared__ double sh[2][kRankThreads / 64];
  double lo = INFINITY, hi = -INFINITY;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < s.A; j += (int64_t)gridDim.x * blockDim.x) {
    if (!s.member(j)) continue;
    const double v = q[j * s.d + s.p];
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fmin(lo, __shfl_down(lo, off, 64));
    hi = fmax(hi, __shfl_down(hi, off, 64));
  }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = lo; sh[1][threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kRankThreads / 64; ++w) { lo = fmin(lo, sh[0][w]); hi = fmax(hi, sh[1][w]); }
    part[2 * blockIdx.x] = lo;
    part[2 * blockIdx.x + 1] = hi;
  }
}

// st[kStConst + series] = 1 when the series' split draws span less than 1e-15 (ArviZ _ess: a constant series)
__global__ void rank_range_final_kernel(int nparts, const double *__restrict__ part, double *__restrict__ flag) {
  if (threadIdx.x != 0) return;
  double lo = INFINITY, hi = -INFINITY;
  for (int b = 0; b < nparts; ++b) { lo = fmin(lo, part[2 * b]); hi = fmax(hi, part[2 * b + 1]); }
  *flag = hi - lo < 1e-15 ? 1.0 : 0.0;
}

// every value of parameter p in the four series (stride d) set to v: a parameter with a non-finite draw
__global__ void __launch_bounds__(kRankThreads)
rank_fill_kernel(RankShape s, double *__restrict__ series, int64_t series_stride, double v) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < s.A; j += (int64_t)gridDim.x * blockDim.x)
    for (int q = 0; q < 4; ++q) series[q * series_stride + j * s.d + s.p] = v;
}

}  // namespace rsfk
