// rsf_kernels_sampler.h — the sampler kernels: mcmc_kernel (float64 RK4, DOP853, and the chain logic alone on supplied sums of
// squares), mcmc_f32x2_kernel (float32 solve, two chains per lane), and probe_adapt_kernel, the self-test of their window
// arithmetic.  Included by rsf_sampler.hip only (probe_adapt_kernel is no template), and by tools/ that build one kernel alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rsf_kernel_common.h"
#include "rsf_device_dop853.h"
#include "rsf_device_f32.h"

namespace rsfk {

// three-parameter sampler: TIGHT loop trips of kD3Trip * kTightUnroll steps like the one-parameter sampler's 2 * (+2.3 %
// over 1 at 131 072 chains x nsteps 4000; the few spills it costs all lie outside the loops)
constexpr int kD3Trip = 2;

// Per-wave statistics of a sampler launch: wave-uniform 32-bit accumulators (scalar registers), added to the ctx totals
// (McmcArgs::stats, 64-bit) by the wave's first lane.  Index = RSF_CNT_* of rsf_abi.h.
constexpr int kFlushEvery = 16;  // rounds between flushes: 16 x 4000 x 8 sub-steps x 64 lanes < 2^32
// tries a lane gets per forward solve to come up with a proposal inside the prior box (mcmc_kernel): with four, at the 39 %
// out-of-bounds rate of the reference's main.py problem 2 % of the lanes still enter a solve idle, for three short rounds
constexpr int kProposalTries = 4;
struct WaveCounters {
  uint32_t accepted, evaluated, nonfinite, oob, early, wave_solves, wave_skips;
  rsf::Wave W;  // the running solve's control, and steps per tier / redone / lane_steps accumulated over the solves
  __device__ __forceinline__ void reset() {
    accepted = evaluated = nonfinite = oob = early = wave_solves = wave_skips = 0;
    W.steps[0] = W.steps[1] = W.steps[2] = W.steps[3] = W.redone = W.lane_steps = W.unguarded = 0;
  }
  __device__ __forceinline__ void flush(unsigned long long *stats) {
    if ((threadIdx.x & 63) == 0) {
      const uint32_t v[RSF_CNT_COUNT] = {accepted, evaluated, nonfinite, oob, early, wave_solves, wave_skips,
                                         W.steps[0], W.steps[1], W.steps[2], W.steps[3], W.redone, W.lane_steps, W.unguarded};
#pragma unroll
      for (int k = 0; k < RSF_CNT_COUNT; ++k)
        if (v[k]) atomicAdd(&stats[k], (unsigned long long)v[k]);
    }
    reset();
  }
};

// Parts of the iteration shared by mcmc_kernel and mcmc_f32x2_kernel (with propose and accept_test above).  A replayed
// variate is element row0 + lane of its [n][C] array: mcmc_kernel passes its lane's own row and lane 0.

// accept / reject, MCMC.py:327-333
template <bool REPLAY>
__device__ __forceinline__ bool metropolis(double ssq, double ssqn, double std2, double lu) {
  return accept_test(REPLAY ? 0.5 * (ssq - ssqn) / std2 : (0.5 * (ssq - ssqn)) * rsf::fm::rcp(std2), lu);
}

// sigma^2 Gibbs update with the post-accept SSq, MCMC.py:158-160
template <bool REPLAY>
__device__ __forceinline__ double gibbs_std2(const McmcArgs &A, uint64_t gid, uint32_t it, int64_t row0, unsigned lane, double std2,
                                             double ssq) {
  const double bval = 0.5 * (A.n0 * std2 + ssq);
  const double g = REPLAY ? (A.g + row0)[lane] : rsf::gamma_draw(A.seed, gid, it, A.gd, A.gc);
  return REPLAY ? bval / g : bval * rsf::fm::rcp(g);
}

// The float64 sampler.  INJECT (rsf_mcmc_replay_ssq): the proposals' sums of squares come from the caller — the chain logic
// alone, no tables, no solve.  Only here: the run-ahead over out-of-bounds proposals (kProposalTries), the uniform drawn before
// the solve for the early-rejection bound thr, the chain state parked in LDS across the solve (kPark), WaveCounters.
template <int D, bool DAMP, bool REPLAY, int MODE, bool INJECT = false>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) mcmc_kernel(Consts K, McmcArgs A) {
  static_assert(MODE == RK4_F64 || MODE == DOP853, "the float32 sampler is mcmc_f32x2_kernel (two chains per lane)");
  static_assert(!INJECT || REPLAY, "supplied sums of squares come with supplied variates");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  rsf::select_group(K);
  // Per-chain arrays are addressed as (wave-uniform row pointer)[threadIdx.x]: the row pointer — array + element * C + the
  // workgroup's first chain — is scalar arithmetic, and the lane's share is one small 32-bit offset, so no access keeps a
  // 64-bit per-lane address alive across the forward solve (with plain [e * C + i] indexing the compiler hoisted two dozen
  // of them out of the iteration loop: 224 B of scratch per lane in the three-parameter kernel).
  const int64_t blk = (int64_t)blockIdx.x * blockDim.x;
  const unsigned t = threadIdx.x;
  const int64_t i = blk + t;
  const bool valid = i < A.C;
  auto at = [&](auto *base, int e) { return base + ((int64_t)e * A.C + blk); };  // wave-uniform
  const bool resident = K.nchunks == 1;

  double q[D];
  double ssq = 0.0, std2 = 1.0;
#pragma unroll
  for (int p = 0; p < D; ++p) q[p] = 1.0;
  // What a proposal needs of the covariance V is its lower Cholesky factor (MCMC.py:497).  D = 1: one double, sqrt(V), kept
  // in a register.  D = 3: the factor's six doubles live in LDS, one slot per lane behind the table chunk (lc[e][lane]:
  // conflict-free), formed from V once per launch and again when the chain adapts.  The adaptation window (D + D + D^2
  // doubles of shifted sums) stays in its HBM arrays and is read-modified-written once per proposal when the chain adapts at
  // all — registers across the forward solve belong to the integrator.  (Until round 4 the one-parameter window sat in
  // registers for the launch: seven of them held across every solve, also when nothing adapts — the BASELINE case — and
  // with them the kernel spilled loop-invariant values whose reload, at the top of every solve, waited for the trace row
  // just stored: vector stores and scratch loads share one counter.)
  double *lcs = lds + A.lc_off + t;  // D = 3: element e of this lane's factor at lcs[e * blockDim.x]
  double V1 = 0.0;                             // D = 1: the proposal variance
  double wr[D], ws[D], wq[D * D];
  int32_t wn = 0;
  auto store_factor = [&](const double *Lf) {  // row-major lower triangle
    int e = 0;
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
      for (int r = 0; r <= p; ++r) lcs[(e++) * blockDim.x] = Lf[p * D + r];
  };
  if (valid) {
#pragma unroll
    for (int p = 0; p < D; ++p) q[p] = at(A.q, p)[t];
    ssq = at(A.ssq, 0)[t];
    std2 = at(A.std2, 0)[t];
  }
  if constexpr (D == 1) {
    if (valid) V1 = at(A.V, 0)[t];
  } else {
    double V[D * D], Lf[D * D];
#pragma unroll
    for (int e = 0; e < D * D; ++e) V[e] = valid ? at(A.V, e)[t] : 0.0;
    rsf::chol_lower<D>(V, Lf);
    store_factor(Lf);
  }
  auto load_window = [&](unsigned t) {
#pragma unroll
    for (int p = 0; p < D; ++p) { wr[p] = at(A.wref, p)[t]; ws[p] = at(A.wsum, p)[t]; }
#pragma unroll
    for (int e = 0; e < D * D; ++e) wq[e] = at(A.wsq, e)[t];
    wn = at(A.wn, 0)[t];
  };
  auto store_window = [&](unsigned t) {
#pragma unroll
    for (int p = 0; p < D; ++p) { at(A.wref, p)[t] = wr[p]; at(A.wsum, p)[t] = ws[p]; }
#pragma unroll
    for (int e = 0; e < D * D; ++e) at(A.wsq, e)[t] = wq[e];
    at(A.wn, 0)[t] = wn;
  };
  // statistics (rsf_mcmc_counters): wave-uniform popcounts and step counts — scalar registers, nothing per lane — added to
  // the ctx totals by one lane every kFlushEvery proposals (32-bit accumulators cannot overflow in between)
  WaveCounters cnt;
  cnt.reset();

  if (resident && !INJECT) {
    if constexpr (MODE == DOP853) rsf::dp::stage_chunk_dp(lds, K, 1, K.nout - 1);
    else rsf::stage_chunk(lds, K, 1, K.nout - 1);
  }

  // The chain's current point, sigma^2, SSq and the logarithm of the accept test's uniform wait out the forward solve in LDS
  // (per-lane slots behind the table chunk; D = 3: behind the Cholesky factor's six) instead of in registers the
  // integrator needs — the spills per proposal these kernels had otherwise.
  constexpr bool kPark = MODE == RK4_F64;  // (the DOP853 kernel allocates worse with it: measured, tools/one_kernel.sh)
  constexpr int kSlotQ = factor_slots(D), kSlotStd2 = kSlotQ + D, kSlotSsq = kSlotStd2 + 1, kSlotLu = kSlotSsq + 1;
  static_assert(kSlotLu + 1 == park_slots(D), "rsf_sampler.hip sizes the launch's LDS with park_slots");

  // Every lane walks its OWN chain through iterations 0 .. n_iters-1 (nl: the lane's next one).  A round of the loop below
  // gives every lane that has no proposal in hand its next one; a proposal outside the prior box is a finished iteration
  // as it stands — rejected without a solve and without a uniform (MCMC.py:318-322), sigma^2 updated, trace row written —
  // so while some lane of the wave came out of bounds and tries are left, the wave closes those iterations and goes round
  // again instead of taking them through a forward solve as idle lanes: with the proposal as wide as the reference's own
  // main.py leaves it (list prior: never adapted, MCMC.py:524-527) four proposals in ten are out of bounds, and a lane
  // that ran ahead this way does a solve's worth of work in every solve.  Lanes that already hold an in-bounds proposal
  // wait out those short rounds.  Nothing about a chain changes: its variates are keyed by (chain, iteration), whichever
  // round draws them.  With replayed variates, or with tables staged chunk by chunk behind workgroup barriers (every
  // wave must then take the same number of solves), there is one try: one iteration per lane and round, as before round 4.
  // The chain state loaded above is complete before the loop starts (the asm reads and redefines the registers): otherwise
  // the loads stay "pending" on the loop's no-solve path as far as the compiler's wait-count bookkeeping can tell, and it
  // guards the first use of sigma^2 and SSq in every round with a wait for ALL vector memory — which at run time is the
  // trace row stored a few instructions earlier (stores and loads share the counter): a store's round trip per round.
#pragma unroll
  for (int p = 0; p < D; ++p) asm volatile("" : "+v"(q[p]));
  asm volatile("" : "+v"(ssq), "+v"(std2), "+v"(V1));
  const int32_t n_iters = (int32_t)A.n_iters;
  const int max_tries = (REPLAY || !resident) ? 1 : kProposalTries;
  int32_t nl = valid ? 0 : n_iters;
  int32_t to_adapt = A.adapt_interval - (int32_t)(A.iter_base % A.adapt_interval);  // closes until the next adaptation is due
  bool have = false;  // an in-bounds proposal (qn, lu, thr) waits for the solve
  double qn[D], lu = 0.0, thr = INFINITY;
#pragma unroll
  for (int p = 0; p < D; ++p) qn[p] = 1.0;
  int tries = 0;
  for (int32_t round = 0;; ++round) {
    const bool todo = nl < n_iters;
    if (resident ? !__any(todo) : round == n_iters) break;
    const uint32_t it = (uint32_t)(A.iter_base + nl);
    // the lane's offset as this round sees it: opaque, so that the addresses built from it are formed where they are
    // used instead of being hoisted out of the loop and kept (or spilled) across every forward solve
    unsigned tl = t;
    asm volatile("" : "+v"(tl));
    const uint64_t gid = (uint64_t)(A.chain_offset + blk + tl);  // RNG is keyed by the GLOBAL chain id
    const int64_t row = (int64_t)nl * A.C + blk + tl;  // this lane's row of the traces / replayed variates
    // ---- proposal, MCMC.py:497 ----
    if (todo && !have) {
      double z[4] = {0.0, 0.0, 0.0, 0.0};
      if (REPLAY) {
#pragma unroll
        for (int p = 0; p < D; ++p) z[p] = A.z[row * D + p];
      } else {
        uint32_t w[4];
        rsf::draw_words(A.seed, gid, it, rsf::SLOT_Z01, w);
        rsf::normal_pair(w, z[0], z[1]);
        if (D > 2) {
          rsf::draw_words(A.seed, gid, it, rsf::SLOT_Z2, w);
          rsf::normal_pair(w, z[2], z[3]);
        }
      }
      if constexpr (D == 1) {
        double Lc;
        rsf::chol_lower<1>(&V1, &Lc);  // sqrt(V), or 0 where V is not positive
        propose<1>(q, [&](int) { return Lc; }, z, qn);
      } else {
        propose<D>(q, [&](int e) { return lcs[e * blockDim.x]; }, z, qn);
      }
      have = in_box<D>(qn, A);
      // ---- the accept test's uniform, drawn before the solve: with it the largest sum of squares that could still be
      // accepted is known, and a lane whose running sum passes it stops holding its wave (rsf::Wave).  thr is that bound
      // widened by 1e-9 (rounding in the test itself is ~1e-16): a lane inside the margin simply integrates to the end.
      lu = 0.0;
      thr = INFINITY;
      if (have) {
        double u;
        if (REPLAY) {
          u = A.u[row];
        } else {
          uint32_t w[4];
          rsf::draw_words(A.seed, gid, it, rsf::SLOT_U, w);
          u = rsf::u53(w[0], w[1]);
        }
        // (replaying recorded variates follows the reference's arithmetic to the last bit: IEEE division, libm-grade log;
        //  the sampler proper uses the kernel's own reciprocal and log — the same value to ~1 ulp)
        lu = REPLAY ? log(u) : rsf::rng_log(u);
        if constexpr (MODE == RK4_F64 && !INJECT) {
          const double t0 = __builtin_fma(-2.0 * std2, lu, ssq);  // accept iff ssqn < ssq - 2 std2 log u, MCMC.py:327-331
          thr = __builtin_fma(1e-9, __builtin_fabs(t0), t0);       // NaN (a chain whose state is not finite): never stops early
        }
      }
    }
    const bool oob = todo && !have;  // this lane's iteration is finished without a solve
    // solve now, unless a lane that just closed an out-of-bounds iteration can still come back with a proposal
    const bool solve_now = tries + 1 >= max_tries || !__any(oob);
    tries = solve_now ? 0 : tries + 1;
    double ssqn = 0.0;
    if (solve_now) {
      const unsigned long long inbmask = rsf::ballot(have);
      cnt.evaluated += (uint32_t)__builtin_popcountll(inbmask);
      if constexpr (!INJECT) {  // (with supplied sums of squares there is no solve to count)
        if (inbmask != 0) ++cnt.wave_solves;
        else ++cnt.wave_skips;
      }
      if constexpr (kPark) {
#pragma unroll
        for (int p = 0; p < D; ++p) lcs[(kSlotQ + p) * blockDim.x] = q[p];
        lcs[kSlotStd2 * blockDim.x] = std2;
        lcs[kSlotSsq * blockDim.x] = ssq;
        lcs[kSlotLu * blockDim.x] = lu;
      }
      // ---- likelihood: forward solve only for in-bounds proposals, MCMC.py:322-324 ----
      double an = K.a_def, bn = K.b_def;
      if constexpr (D == 3) { an = qn[1]; bn = qn[2]; }
      // (a wave with no in-bounds lane skips the solve when the tables are resident: no barrier inside)
      if constexpr (INJECT) {
        if (have) ssqn = A.ssq_new[row];
      } else if (!resident || inbmask != 0) {
        if constexpr (MODE == DOP853) {
          ssqn = rsf::dp::solve<DAMP, true, false>(lds, K, resident, have, qn[0], an, bn, nullptr, 0);
        } else {
          ssqn = rsf::solve<DAMP, true, false, (D == 1 ? 2 : kD3Trip) * rsf::kTightUnroll, true>(lds, K, resident, have, qn[0], an, bn, thr, nullptr, 0, cnt.W);
          cnt.early += (uint32_t)__builtin_popcountll(inbmask & ~cnt.W.alive);
        }
      }
      if constexpr (kPark) {
        // opaque: the values are re-read, not carried across the solve.  The OFFSET is laundered, not the pointer: a pointer
        // that went through the asm has lost its address space and is read back with flat loads, which sit on the
        // vector-memory counter too — the wait for them then also waits for the trace row stored just before.
        unsigned relaunder = 0;
        asm volatile("" : "+v"(relaunder));
        const double *back = lcs + relaunder;
#pragma unroll
        for (int p = 0; p < D; ++p) q[p] = back[(kSlotQ + p) * blockDim.x];
        std2 = back[kSlotStd2 * blockDim.x];
        ssq = back[kSlotSsq * blockDim.x];
        lu = back[kSlotLu * blockDim.x];
      }
    }
    // ---- close the iteration: of the lanes that were solved, and of the lanes whose proposal was out of bounds ----
    const bool solved = solve_now && have;
    // accept / reject, MCMC.py:327-333
    bool accept = false;
    if (solved) {
      accept = metropolis<REPLAY>(ssq, ssqn, std2, lu);
      if (accept) {
        ssq = ssqn;
#pragma unroll
        for (int p = 0; p < D; ++p) q[p] = qn[p];
      }
    }
    cnt.accepted += (uint32_t)__builtin_popcountll(rsf::ballot(accept));
    cnt.nonfinite += (uint32_t)__builtin_popcountll(rsf::ballot(solved && !isfinite(ssqn)));
    cnt.oob += (uint32_t)__builtin_popcountll(rsf::ballot(oob));
    if (solved || oob) {
      // sigma^2 Gibbs update with the post-accept SSq, MCMC.py:158-160
      std2 = gibbs_std2<REPLAY>(A, gid, it, row, 0, std2, ssq);
      if (A.tq) {
#pragma unroll
        for (int p = 0; p < D; ++p) A.tq[row * D + p] = q[p];
      }
      if (A.ts) A.ts[row] = std2;
      if (A.ta) A.ta[row] = accept ? 1 : 0;
      // adaptation, MCMC.py:200-204, 523-527
      if (A.adapt_mode != RSF_ADAPT_NONE) {
        load_window(tl);
#pragma unroll
        for (int p = 0; p < D; ++p) {
          ws[p] += q[p] - wr[p];
#pragma unroll
          for (int r = 0; r < D; ++r) wq[p * D + r] += (q[p] - wr[p]) * (q[r] - wr[r]);
        }
        ++wn;
        if (A.adapt_mode == RSF_ADAPT_REFERENCE_DICT) at(A.wbuf, A.adapt_interval - to_adapt)[tl] = q[0];  // slot (iteration % interval)
        if (--to_adapt == 0) {
          to_adapt = A.adapt_interval;
          if (wn >= 2) {
            const double nn = (double)wn;
            double Vn[D * D], Ln[D * D];
            if (A.adapt_mode == RSF_ADAPT_REFERENCE_DICT) {
              // d := len(qpriors.keys()) (2 for {1: lo, 2: hi}), and the Cholesky FACTOR becomes the next covariance
              // (one-parameter chains only: rsf_mcmc_init refuses the mode for D = 3).  The window's covariance in np.cov's own
              // arithmetic, from the samples kept in wbuf (full and in order whenever an adaptation is due).
              Vn[0] = A.dict_scale * rsf::np_cov_1d([&](int k) { return at(A.wbuf, k)[tl]; }, A.adapt_interval);
              if (rsf::chol_lower<1>(Vn, Ln)) V1 = Ln[0];
            } else if (rsf::window_covariance<D>(ws, wq, nn, 2.38 * 2.38 / (double)D, A.am_eps, Vn, Ln)) {
              if constexpr (D == 1) {
                V1 = Vn[0];
              } else {
#pragma unroll
                for (int e = 0; e < D * D; ++e) at(A.V, e)[tl] = Vn[e];
                store_factor(Ln);
              }
            }
          }
          // (am keeps its sums: the covariance of the whole history.  reference_dict forms its window from wbuf and ignores them.)
        }
        store_window(tl);
      }
      ++nl;
      have = false;
    }
    if ((round & (kFlushEvery - 1)) == kFlushEvery - 1) cnt.flush(A.stats);
  }

  if (valid) {
#pragma unroll
    for (int p = 0; p < D; ++p) at(A.q, p)[t] = q[p];
    if constexpr (D == 1) at(A.V, 0)[t] = V1;
    at(A.ssq, 0)[t] = ssq;
    at(A.std2, 0)[t] = std2;
  }
  cnt.flush(A.stats);
}

// The float32 sampler (RSF_FLAG_FP32_SOLVE): the same iteration as mcmc_kernel, with TWO chains per lane, because its
// solve advances two chains per packed instruction (rsf_device_f32.h, solve32x2).  Chain slot s of lane t of workgroup w
// is chain w * 2 * blockDim + s * blockDim + t, so that both slots read and write coalesced runs.  (A second kernel
// rather than a chains-per-lane parameter of mcmc_kernel: written that way, the float64 kernels — which sit at 252-256
// registers — came out with 12-44 B of scratch per lane.)  The sampler logic itself stays float64, with mcmc_kernel's
// propose, metropolis and gibbs_std2.  Only here: the uniform is drawn after the solve, the one-parameter window stays in
// registers, counters are reduced once (wave_sum).  The draws, box test, trace row and adaptation are still written
// out in both kernels: as helpers they grew this kernel's spills (d = 3: 512 -> 528-1008 B, the adaptation's partly inside
// the trip loop) or mcmc_kernel's SGPR spills in its solve loops (HISTORY.md: one definition of the chain logic).
// Per-chain sampler state of one slot:
template <int D>
struct Chain {
  double q[D], ssq, std2;
  double V1;                   // D = 1: the proposal variance
  double wr[D], ws[D], wq[D * D];  // adaptation window (D = 1 only: held in registers for the launch)
  int32_t wn;
  bool valid;
  uint64_t gid;                // RNG is keyed by the GLOBAL chain id
};

template <int D, bool DAMP, bool REPLAY>
__global__ void __launch_bounds__(kMaxBlock, kMinBlocks) __attribute__((amdgpu_num_vgpr(RSF_F32_TRIP_COMPILER_VGPRS / 2)))
mcmc_f32x2_kernel(Consts K, McmcArgs A) {  // (the registers above that count: the solve's private file, rsf_device_f32.h trip32)
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int NC = 2;  // chains per lane
  // Per-chain arrays are addressed as (wave-uniform row pointer)[threadIdx.x]: the row pointer — array + element * C + the
  // slot's first chain — is scalar arithmetic, and the lane's share is one small 32-bit offset, so no access keeps a
  // 64-bit per-lane address alive across the forward solve (with plain [e * C + i] indexing the compiler hoisted two dozen
  // of them out of the iteration loop: 224 B of scratch per lane in the three-parameter kernel).
  const int64_t blk = (int64_t)blockIdx.x * blockDim.x * NC;  // first chain of this workgroup
  if (K.group_chains > 0) K.data += (blk / K.group_chains) * K.nout;  // the observation series of the workgroup's chain group
  const unsigned t = threadIdx.x;
  auto at = [&](auto *base, int e, int s) { return base + ((int64_t)e * A.C + blk + (int64_t)s * blockDim.x); };  // wave-uniform
  const bool resident = K.nchunks == 1;

  // What a proposal needs of the covariance V is its lower Cholesky factor (MCMC.py:497).  D = 1: one double, sqrt(V), kept
  // in a register with the three doubles of the adaptation window.  D = 3: the factor's six doubles live in LDS, one slot
  // per chain behind the table chunk (lc[e][slot][lane]: conflict-free), formed from V once per launch and again when the
  // chain adapts; the window (3 + 3 + 9 doubles of shifted sums) stays in its HBM arrays and is read-modified-written once
  // per proposal when the chain adapts at all — registers across the forward solve belong to the integrator.
  constexpr bool kWinRegs = D == 1;
  double *lcs = lds + A.lc_off + t;  // D = 3: element e of slot s's factor at lcs[(e * NC + s) * blockDim.x]
  Chain<D> ch[NC];
  auto store_factor = [&](int s, const double *Lf) {  // row-major lower triangle
    int e = 0;
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
      for (int r = 0; r <= p; ++r) lcs[((e++) * NC + s) * blockDim.x] = Lf[p * D + r];
  };
  auto load_window = [&](int s, unsigned t) {
    Chain<D> &c = ch[s];
#pragma unroll
    for (int p = 0; p < D; ++p) { c.wr[p] = at(A.wref, p, s)[t]; c.ws[p] = at(A.wsum, p, s)[t]; }
#pragma unroll
    for (int e = 0; e < D * D; ++e) c.wq[e] = at(A.wsq, e, s)[t];
    c.wn = at(A.wn, 0, s)[t];
  };
  auto store_window = [&](int s, unsigned t) {
    const Chain<D> &c = ch[s];
#pragma unroll
    for (int p = 0; p < D; ++p) { at(A.wref, p, s)[t] = c.wr[p]; at(A.wsum, p, s)[t] = c.ws[p]; }
#pragma unroll
    for (int e = 0; e < D * D; ++e) at(A.wsq, e, s)[t] = c.wq[e];
    at(A.wn, 0, s)[t] = c.wn;
  };
#pragma unroll
  for (int s = 0; s < NC; ++s) {
    Chain<D> &c = ch[s];
    const int64_t i = blk + (int64_t)s * blockDim.x + t;
    c.valid = i < A.C;
    c.gid = (uint64_t)(A.chain_offset + i);
    c.ssq = 0.0; c.std2 = 1.0; c.V1 = 0.0; c.wn = 0;
#pragma unroll
    for (int p = 0; p < D; ++p) c.q[p] = 1.0;
    if (c.valid) {
#pragma unroll
      for (int p = 0; p < D; ++p) c.q[p] = at(A.q, p, s)[t];
      c.ssq = at(A.ssq, 0, s)[t];
      c.std2 = at(A.std2, 0, s)[t];
    }
    if constexpr (D == 1) {
      if (c.valid) c.V1 = at(A.V, 0, s)[t];
    } else {
      double V[D * D], Lf[D * D];
#pragma unroll
      for (int e = 0; e < D * D; ++e) V[e] = c.valid ? at(A.V, e, s)[t] : 0.0;
      rsf::chol_lower<D>(V, Lf);
      store_factor(s, Lf);
    }
    if (kWinRegs && A.adapt_mode != RSF_ADAPT_NONE && c.valid) load_window(s, t);
  }
  uint32_t n_acc = 0, n_eval = 0, n_nonfinite = 0, n_oob = 0, n_solves = 0;
  rsf::f32::Trips32 trips;  // wave-uniform: what the wave's solves ran (steps_tight = incremental, steps_full, steps_redone)

  float *lds32 = reinterpret_cast<float *>(lds);
  if (resident) rsf::f32::stage_chunk32(lds32, K, 1, K.nout - 1);

  for (int64_t n = 0; n < A.n_iters; ++n) {
    const uint32_t it = (uint32_t)(A.iter_base + n);
    // the lane's offset as this iteration sees it: opaque, so that the addresses built from it are formed where they are
    // used instead of being hoisted out of the loop and kept (or spilled) across every forward solve
    unsigned tl = t;
    asm volatile("" : "+v"(tl));
    double qn[NC][D], ssqn[NC];
    bool inb[NC];
    // ---- proposal, MCMC.py:497 ----
#pragma unroll
    for (int s = 0; s < NC; ++s) {
      const Chain<D> &c = ch[s];
      const int64_t row0 = n * A.C + blk + (int64_t)s * blockDim.x;  // trace row of the slot's first chain (wave-uniform)
      double z[4] = {0.0, 0.0, 0.0, 0.0};
      if (REPLAY) {
        if (c.valid) {
#pragma unroll
          for (int p = 0; p < D; ++p) z[p] = (A.z + row0 * D)[tl * D + p];
        }
      } else {
        uint32_t w[4];
        rsf::draw_words(A.seed, c.gid, it, rsf::SLOT_Z01, w);
        rsf::normal_pair(w, z[0], z[1]);
        if (D > 2) {
          rsf::draw_words(A.seed, c.gid, it, rsf::SLOT_Z2, w);
          rsf::normal_pair(w, z[2], z[3]);
        }
      }
      if constexpr (D == 1) {
        double Lc;
        rsf::chol_lower<1>(&c.V1, &Lc);  // sqrt(V), or 0 where V is not positive
        propose<1>(c.q, [&](int) { return Lc; }, z, qn[s]);
      } else {
        propose<D>(c.q, [&](int e) { return lcs[(e * NC + s) * blockDim.x]; }, z, qn[s]);
      }
      inb[s] = c.valid;
#pragma unroll
      for (int p = 0; p < D; ++p) inb[s] = inb[s] && (qn[s][p] > A.lo[p]) && (qn[s][p] < A.hi[p]);  // strict box, MCMC.py:318-320
      if (c.valid && !inb[s]) ++n_oob;
      ssqn[s] = 0.0;
    }
    // ---- likelihood: forward solve only for in-bounds proposals, MCMC.py:322-324 ----
    // (a wave with no in-bounds lane skips the solve when the tables are resident: no barrier inside)
    if (!resident || __any(inb[0] || inb[1])) {
      double dcn[2], an[2], bn[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) { dcn[s] = qn[s][0]; an[s] = D == 3 ? qn[s][D - 2] : K.a_def; bn[s] = D == 3 ? qn[s][D - 1] : K.b_def; }
      rsf::f32::solve32x2<DAMP>(lds32, K, resident, inb, dcn, an, bn, ssqn, trips);
      ++n_solves;
    }
#pragma unroll
    for (int s = 0; s < NC; ++s) {
      Chain<D> &c = ch[s];
      const int64_t row0 = n * A.C + blk + (int64_t)s * blockDim.x;
      // ---- accept / reject, MCMC.py:327-333 ----
      bool accept = false;
      if (inb[s]) {
        double u;
        if (REPLAY) {
          u = (A.u + row0)[tl];
        } else {
          uint32_t w[4];
          rsf::draw_words(A.seed, c.gid, it, rsf::SLOT_U, w);
          u = rsf::u53(w[0], w[1]);
        }
        // (log u as in mcmc_kernel)
        accept = metropolis<REPLAY>(c.ssq, ssqn[s], c.std2, REPLAY ? log(u) : rsf::rng_log(u));
        ++n_eval;
        if (!isfinite(ssqn[s])) ++n_nonfinite;
        if (accept) {
          c.ssq = ssqn[s];
#pragma unroll
          for (int p = 0; p < D; ++p) c.q[p] = qn[s][p];
          ++n_acc;
        }
      }
      // ---- sigma^2 Gibbs update with the post-accept SSq, MCMC.py:158-160 ----
      if (c.valid) {
        c.std2 = gibbs_std2<REPLAY>(A, c.gid, it, row0, tl, c.std2, c.ssq);
        if (A.tq) {
#pragma unroll
          for (int p = 0; p < D; ++p) (A.tq + row0 * D)[tl * D + p] = c.q[p];
        }
        if (A.ts) (A.ts + row0)[tl] = c.std2;
        if (A.ta) (A.ta + row0)[tl] = accept ? 1 : 0;
      }
      // ---- adaptation, MCMC.py:200-204, 523-527 ----
      if (A.adapt_mode != RSF_ADAPT_NONE && c.valid) {
        if (!kWinRegs) load_window(s, tl);
#pragma unroll
        for (int p = 0; p < D; ++p) {
          c.ws[p] += c.q[p] - c.wr[p];
#pragma unroll
          for (int r = 0; r < D; ++r) c.wq[p * D + r] += (c.q[p] - c.wr[p]) * (c.q[r] - c.wr[r]);
        }
        ++c.wn;
        if (A.adapt_mode == RSF_ADAPT_REFERENCE_DICT) at(A.wbuf, (int)((A.iter_base + n) % A.adapt_interval), s)[tl] = c.q[0];
        if ((A.iter_base + n + 1) % A.adapt_interval == 0) {
          if (c.wn >= 2) {
            const double nn = (double)c.wn;
            double Vn[D * D], Ln[D * D];
            if (A.adapt_mode == RSF_ADAPT_REFERENCE_DICT) {
              // d := len(qpriors.keys()) (2 for {1: lo, 2: hi}), and the Cholesky FACTOR becomes the next covariance
              // (one-parameter chains only: rsf_mcmc_init refuses the mode for D = 3); np.cov's own arithmetic (mcmc_kernel)
              Vn[0] = A.dict_scale * rsf::np_cov_1d([&](int k) { return at(A.wbuf, k, s)[tl]; }, A.adapt_interval);
              if (rsf::chol_lower<1>(Vn, Ln)) c.V1 = Ln[0];
            } else if (rsf::window_covariance<D>(c.ws, c.wq, nn, 2.38 * 2.38 / (double)D, A.am_eps, Vn, Ln)) {
              if constexpr (D == 1) {
                c.V1 = Vn[0];
              } else {
#pragma unroll
                for (int e = 0; e < D * D; ++e) at(A.V, e, s)[tl] = Vn[e];
                store_factor(s, Ln);
              }
            }
          }
          // (am keeps its sums: the covariance of the whole history; mcmc_kernel)
        }
        if (!kWinRegs) store_window(s, tl);
      }
    }
  }

#pragma unroll
  for (int s = 0; s < NC; ++s) {
    const Chain<D> &c = ch[s];
    if (c.valid) {
#pragma unroll
      for (int p = 0; p < D; ++p) at(A.q, p, s)[t] = c.q[p];
      if constexpr (D == 1) at(A.V, 0, s)[t] = c.V1;
      at(A.ssq, 0, s)[t] = c.ssq;
      at(A.std2, 0, s)[t] = c.std2;
      if (kWinRegs && A.adapt_mode != RSF_ADAPT_NONE) store_window(s, t);
    }
  }
  // statistics: wave shuffle reduction, one atomic per wave and counter
  const unsigned long long s0 = wave_sum<unsigned long long>(n_acc), s1 = wave_sum<unsigned long long>(n_eval),
                           s2 = wave_sum<unsigned long long>(n_nonfinite), s3 = wave_sum<unsigned long long>(n_oob);  // 64-bit sums of the 32-bit counters
  if ((threadIdx.x & 63) == 0) {
    if (s0) atomicAdd(&A.stats[RSF_CNT_ACCEPTED], s0);
    if (s1) atomicAdd(&A.stats[RSF_CNT_EVALUATED], s1);
    if (s2) atomicAdd(&A.stats[RSF_CNT_NONFINITE], s2);
    if (s3) atomicAdd(&A.stats[RSF_CNT_OUT_OF_BOUNDS], s3);
    if (n_solves) atomicAdd(&A.stats[RSF_CNT_WAVE_SOLVES], (unsigned long long)n_solves);
    if (trips.incr) atomicAdd(&A.stats[RSF_CNT_STEPS_TIGHT], (unsigned long long)trips.incr);
    if (trips.full) atomicAdd(&A.stats[RSF_CNT_STEPS_FULL], (unsigned long long)trips.full);
    if (trips.redone) atomicAdd(&A.stats[RSF_CNT_STEPS_REDONE], (unsigned long long)trips.redone);
  }
}

// rsf_mcmc_adapt: update_covariance_matrix (MCMC.py:200-204) of a window of samples win[n][d] with the sampler's own arithmetic
// (shifted sums about the window's first sample, rsf::window_covariance).  out[0 .. d*d) = the next "Vold" of the
// reference's loop — reference_dict: the Cholesky FACTOR (MCMC.py:203-204, 525); am: the covariance — out[d*d] = 1 if
// positive definite, else 0.
template <int D>
__device__ void adapt_window(int n, const double *win, int mode, double dict_scale, double *out) {
  double ws[D], wq[D * D], Vn[D * D], Ln[D * D];
#pragma unroll
  for (int p = 0; p < D; ++p) ws[p] = 0.0;
#pragma unroll
  for (int e = 0; e < D * D; ++e) wq[e] = 0.0;
  for (int k = 0; k < n; ++k)
#pragma unroll
    for (int p = 0; p < D; ++p) {
      ws[p] += win[k * D + p] - win[p];
#pragma unroll
      for (int r = 0; r < D; ++r) wq[p * D + r] += (win[k * D + p] - win[p]) * (win[k * D + r] - win[r]);
    }
  const bool dict = mode == RSF_ADAPT_REFERENCE_DICT;
  bool ok = n >= 2;
  if (dict) {  // one parameter: np.cov's own arithmetic, like the sampler's
    Vn[0] = ok ? dict_scale * rsf::np_cov_1d([&](int k) { return win[k * D]; }, n) : 0.0;
    ok = ok && rsf::chol_lower<1>(Vn, Ln);
  } else {
    const double no_eps[3] = {0.0, 0.0, 0.0};  // the given samples alone: what the sampler computes once its history is these
    ok = ok && rsf::window_covariance<D>(ws, wq, (double)n, 2.38 * 2.38 / (double)D, no_eps, Vn, Ln);
  }
#pragma unroll
  for (int e = 0; e < D * D; ++e) out[e] = dict ? Ln[e] : Vn[e];
  out[D * D] = ok ? 1.0 : 0.0;
}

__global__ void probe_adapt_kernel(int d, int n, const double *win, int mode, double dict_scale, double *out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (d == 1) adapt_window<1>(n, win, mode, dict_scale, out);
  else adapt_window<3>(n, win, mode, dict_scale, out);
}

}  // namespace rsfk
