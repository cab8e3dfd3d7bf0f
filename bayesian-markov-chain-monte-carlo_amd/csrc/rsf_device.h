// rsf_device.h — device-side building blocks of the gfx950 kernels (included by the units of csrc/ through the kernel headers; no kernel is defined here).
//
//   Philox4x32-10 counter RNG + Box-Muller normals + Marsaglia-Tsang gamma   (K3)
//   rate-and-state friction RHS and the classical RK4 step, per lane          (K1 core)
//     hot path: 8-16 steps per loop trip, transcendentals carried incrementally (rk4_tight / integrate_multi; the
//               remainder in pairs, integrate_pairs)
//     cold path: full log/exp evaluation (rk4_cold), taken when an increment leaves the series' guard region
//   cooperative LDS staging of the chain-independent tables (loading V_l(t), observation)
//
// One lane integrates one chain; a wave64 is 64 independent chains.  The time recurrence is
// sequential, so the sum of squares is a per-lane running sum; cross-lane work is confined to
// the statistics counters (wave shuffle reduction) and LDS broadcast reads of the tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rsf_math.h"

namespace rsf {

// ---------------------------------------------------------------------------------------------
// Kernel-argument blocks (wave-uniform → live in SGPRs)
// ---------------------------------------------------------------------------------------------
struct Consts {
  double mu_ref, V_ref, k1, mu0;  // RateStateModel.py:167-180
  double a_def, b_def;            // model.a / model.b where no per-lane value is given
  double h, hh, h6;               // RK4 step, h/2, h/6
  double inv_dt;                  // 1 / delta_t
  double t0, dt;                  // t_start, delta_t
  double inv_vref;                // 1/V_ref
  double cacc;                    // (h/6)/delta_t: acceleration sample = cacc * (k1 + 2 k2 + 2 k3 + k4)_V summed over the interval
  const double *vl;               // V_l at stage times t_start + j*h/2, j = 0 .. 2*S*(nout-1)
  const double *data;             // observation [nout] (of this workgroup's chain group) or nullptr
  int64_t group_chains;           // chains per observation group (0: one series for all)
  int32_t nout;                   // output samples (RateStateModel.py:358)
  int32_t S;                      // RK4 steps per output interval
  int32_t kc;                     // output intervals per LDS chunk
  int32_t nchunks;                // ceil((nout-1)/kc); 1 => tables stay resident in LDS
  double vl_lo, vl_hi;            // smallest and largest value of vl over the whole series (the host's, where it writes the table):
                                  //   what tight_needs_guard knows of the loading.  Last, so that no other field moves.
};

// select the observation series of this workgroup (all its chains belong to one group)
__device__ __forceinline__ void select_group(Consts &K) {
  if (K.group_chains > 0) K.data += ((int64_t)blockIdx.x * blockDim.x / K.group_chains) * K.nout;
}

// Per-lane proposal constants, hoisted out of the time loop.  The integrator works on the rescaled state
//   ms = mu / k'      (k' = 1e-2*10/Dc, RateStateModel.py:324)      x = V_ref theta / Dc
// — a linear change of variables, so RK4 produces the same trajectory to rounding — because two
// multiplications then drop out of every RHS evaluation: d(ms)/dt = V_l - v and d(theta)/dt = 1 - w x
// (w = v/V_ref, so w x = v theta/Dc, and log(V_ref theta/Dc) = log x).
struct Lane {
  double inv_dc;  // 1/Dc
  double vdc;     // V_ref/Dc      : dx/dt = vdc * d1
  double kprime;  // k'
  double kia;     // k'/a          : d(mu)/a = kia * d(ms)
  double khh, kh, kh6;  // kia*(h/2), kia*h, kia*(h/6): d(mu)/a of a stage / step straight from the ms derivative
  // dV/dt = (v/a)(dmu/dt - b/theta dtheta/dt) = vk w g with g = d0 - beta d1/x (d0 = V_l - v = d(ms)/dt): the integrator works on
  // g, i.e. on dV/dt in units of vk per unit w — vk multiplies only the finished sample (cv), not every stage
  double vk;      // (V_ref/a) k'
  double beta;    // (b/theta dtheta/dt)/(k' d(ms)/dt) coefficient: (V_ref b/Dc)/k' = 10 b V_ref (independent of Dc)
  double kvk;     // (k1/k') vk = k1 V_ref/a : radiation damping, d0 -= kvk w g
  // With radiation damping the incremental tiers carry W = kvk w in place of w (tier_enter): w enters every use there
  // linearly through a per-lane constant, so the constants absorb 1/kvk and the damping pass needs no product.  The
  // steps' V-derivative sums are then in units of vk/kvk (the cold step's too: rhs_tail), and cv / h6v include the 1/kvk.
  // Without damping W = w and these are the plain constants.
  double vrw;     // V_ref/kvk     : d0 = V_l - vrw W
  double hhdw, hdw;  // hhd/kvk, hd/kvk: the xr forms of rk4_tight
  double cv;      // cacc vk / kvk : acceleration sample = cv * (g-weighted RK4 sum of the step)
  double h6v;     // (h/6) vk / kvk: velocity increment of a step = h6v * that sum
  double boa;     // b/a
  double nhboa;   // -b/2a : (b/a) log1p(rho) = rho (b/a - (b/2a) rho) in the TIGHT tier, two fmas with dlt
  double tc;      // -mu_ref/a
  double hhd, hd, h6d;  // (h/2)/Dc, h/Dc, (h/6)/Dc : theta increments in x units
  double bh;            // beta/hhd: the TIGHT tier carries hhd/x in place of 1/x (rk4_tight)
  double c_l1p, c_l1q;  // series coefficients of the active tier kept in VGPRs (a VOP3 takes one SGPR source and the first Horner
  double c_em1;         //   term has two non-inline constants), see set_tier: b/3a and -b/4a of log1p, expm1's leading coefficient
  // the in-step sum of squares (rk4_tight, INSTEP): the sample's residual straight from the step's two partial sums, and the
  // full-step stage fed with the half increment c1 (rho = 2 c1) through doubled constants (the step's other in-step constants
  // are formed where its loops are entered: struct Series)
  double cv2;           // 2 cv
  double bh2;           // -2 bh: the full-step stage's bracket, bh (1 - rho) = bh + c1 (-2 bh) (tight_incr_scaled)
};

template <int T>
__device__ __forceinline__ void set_tier(Lane &L);

// DAMP: radiation damping, k1 != 0 (with k1 = 0 the host launches the DAMP = false kernels: the damping pass is then an exact
// identity, and W = kvk w would be 0)
// STIFF (rsf_kernels_stiff.h, include/rsf_stiff.h): the spring's stiffness k is the caller's, independent of Dc — kappa = k Dc
// stands where the reference's coupling has the literal 1e-2 * 10, ikappa = 1 / kappa (one IEEE division per lane per solve, the
// caller's) where it has that literal's reciprocal; every other constant is formed as it is.  Without STIFF the two are not read.
template <bool DAMP, bool STIFF = false>
__device__ __forceinline__ Lane make_lane(double dc, double a, double b, const Consts &K, double kappa = 0.0, double ikappa = 0.0) {
  Lane L;
  // reciprocals by rsf_math.h (<= 1 ulp from the IEEE quotient at a fifth of its instruction count)
  const double inv_a = fm::rcp(a);
  L.inv_dc = fm::rcp(dc);
  if constexpr (STIFF) L.kprime = kappa * L.inv_dc;
  else L.kprime = (1e-2 * 10) * L.inv_dc;
  L.kia = L.kprime * inv_a;
  L.khh = L.kia * K.hh;
  L.kh = L.kia * K.h;
  L.kh6 = L.kia * K.h6;
  const double via = K.V_ref * inv_a;
  L.vdc = K.V_ref * L.inv_dc;
  L.vk = via * L.kprime;
  if constexpr (STIFF) L.beta = (b * K.V_ref) * ikappa;
  else L.beta = (b * K.V_ref) * (1.0 / (1e-2 * 10));
  L.kvk = K.k1 * via;
  const double ikw = DAMP ? fm::rcp(L.kvk) : 1.0;
  const double vkw = DAMP ? L.vk * ikw : L.vk;
  L.cv = K.cacc * vkw;
  L.h6v = K.h6 * vkw;
  L.boa = b * inv_a;
  L.tc = -K.mu_ref * inv_a;
  L.hhd = K.hh * L.vdc;
  L.hd = K.h * L.vdc;
  L.h6d = K.h6 * L.vdc;
  L.vrw = DAMP ? K.V_ref * ikw : K.V_ref;
  L.hhdw = DAMP ? L.hhd * ikw : L.hhd;
  L.hdw = DAMP ? L.hd * ikw : L.hd;
  L.nhboa = -0.5 * L.boa;
  L.bh = L.beta * fm::rcp(L.hhd);
  L.cv2 = 2.0 * L.cv;  // (exact doublings; formed only where an instantiation reads them)
  L.bh2 = -2.0 * L.bh;
  set_tier<2>(L);
  return L;
}

// ---------------------------------------------------------------------------------------------
// RHS, RateStateModel.py:318-355.  y[2] (V) never feeds back, so only (mu, theta) are inputs.
// Same quantities as the reference, regrouped so that every reciprocal is hoisted into Lane and
// the slip rate appears only as w = v/V_ref = exp((mu-mu_ref)/a - (b/a) log(V_ref*theta/Dc)).
// ---------------------------------------------------------------------------------------------

// Integration state of one lane: ms = mu/k', x = V_ref theta/Dc, V, and the transcendental parts of the RHS at
// that point:  w = v/V_ref = exp(mu/a - mu_ref/a - (b/a) log x),   rx = 1/x.
// INSIDE the TIGHT tier's loops rx holds Rh = hhd/x instead and x is NOT carried (tier_enter / tier_leave): the step-end
// update 1/x' = (1/x)(1 + q) is indifferent to a constant factor, the tier's step works on theta derivatives scaled by
// Rh and never reads x itself (rk4_tight); where x is needed — a resync, a cold trip, leaving the tier — it is hhd / Rh.
// With radiation damping w is carried there as W = kvk w as well (Lane::vrw).
struct State {
  double ms, x, V;
  double w, rx;
};

// the RHS once w and 1/x are known.  d0 = d(ms)/dt, d1 = d(theta)/dt (so dx = d1/Dc), d2 = (dV/dt)/vk — with damping
// (dV/dt) kvk/vk, the units of the incremental tiers' sums (Lane::vrw), from the product the damping pass forms anyway.
template <bool DAMP>
__device__ __forceinline__ void rhs_tail(double w, double rx, double x, double vl, const Lane &L,
                                         const Consts &K, double &d0, double &d1, double &d2) {
  d1 = __builtin_fma(-w, x, 1.0);                    // ageing law: 1 - v*theta/Dc
  d0 = __builtin_fma(-K.V_ref, w, vl);               // spring loading / k':  V_l - v
  const double bt = (L.beta * d1) * rx;              // b/theta * dtheta/dt, in units of k'
  double g = d0 - bt;                                // dV/dt = vk w g:  v/a (dmu/dt - b/theta dtheta/dt), RateStateModel.py:346
  if (DAMP) {                                        // one fixed-point pass, RateStateModel.py:349-353: d0 -= k1/k' * dV/dt,
    const double kw = L.kvk * w;                     //   then dV/dt again
    d0 = __builtin_fma(-kw, g, d0);
    g = d0 - bt;
    d2 = kw * g;
  } else {
    d2 = w * g;
  }
}

// (w, 1/x) by full evaluation
__device__ __forceinline__ void eval_full(double ms, double x, const Lane &L, const Consts &K, double &w, double &rx) {
  w = fm::exp(__builtin_fma(-L.boa, fm::log(x), __builtin_fma(ms, L.kia, L.tc)));
  rx = fm::rcp(x);
}

enum Tier : int { TIGHT = 0, NARROW = 1, WIDE = 2, FULL = 3 };  // FULL: a full evaluation at every stage (struct Wave)

// a value formed where it is used: opaque to common-subexpression elimination and hoisting, so that it holds no register
// through the loops (1/hhd and 1/kvk, needed only where a lane leaves the incremental tiers)
__device__ __forceinline__ double local_value(double x) {
  asm volatile("" : "+v"(x));
  return x;
}

// the incremental tiers' representation of 1/x and w (struct State, Lane::vrw)
template <bool DAMP, int T>
__device__ __forceinline__ void tier_enter(State &s, const Lane &L) {
  s.rx *= L.hhd;
  if (DAMP) s.w *= L.kvk;
}
template <int T>
__device__ __forceinline__ void tier_x(State &s, const Lane &L) { s.x = L.hhd * fm::rcp(s.rx); }  // x from Rh
template <bool DAMP, int T>
__device__ __forceinline__ void tier_leave(State &s, const Lane &L) {
  tier_x<T>(s, L);
  s.rx *= fm::rcp(local_value(L.hhd));
  if (DAMP) s.w *= fm::rcp(local_value(L.kvk));
}
template <bool DAMP, int T>
__device__ __forceinline__ void eval_full_t(State &s, const Lane &L, const Consts &K) {  // from (ms, x)
  eval_full(s.ms, s.x, L, K, s.w, s.rx);
  tier_enter<DAMP, T>(s, L);
}
template <bool DAMP, int T>
__device__ __forceinline__ void resync_t(State &s, const Lane &L, const Consts &K) {  // inside tier T's loop
  tier_x<T>(s, L);
  eval_full_t<DAMP, T>(s, L, K);
}

// ms from the incremental tiers' (W, Rh): the inverse of eval_full on the scaled state,
//     ms = (log w - tc + (b/a) log x) / kia,   x = hhd / Rh,  w = W / kvk with damping.
// The in-step TIGHT trips do not carry ms (rk4_tight, INSTEP; Wave::ms_stale): whoever reads it after them forms it here first.
// Every constant is formed where it is used (local_value), so nothing of this is live through a loop.  Measured against long
// double on the lanes of tests/test_ms_free.py (the NumPy restatement): ms comes back within 1.04 ulp.
template <bool DAMP>
__device__ __forceinline__ void rebuild_ms(State &s, const Lane &L) {
  const double lx = fm::log(local_value(L.hhd) * fm::rcp(s.rx));
  const double lw = fm::log(DAMP ? s.w * fm::rcp(local_value(L.kvk)) : s.w);
  s.ms = (__builtin_fma(local_value(L.boa), lx, lw) - local_value(L.tc)) * fm::rcp(local_value(L.kia));
}

// (w', 1/x') at (ms + dms, x1 = x + dx) from (w, rx) at (ms, x).  With rho = dx/x (= dtheta/theta) and
// dlt = dk - (b/a) log1p(rho), dk = dmu/a = kia*dms:   w' = w exp(dlt),   1/x' = (1/x)/(1 + rho),
// by short series — the same function of (ms', x') to rounding inside the tier's guard region:
//   tier     |rho| <   |dlt| <   log1p to     expm1 to       1/x' = (1/x)(1 + q), q =                 truncation
//   TIGHT    2^-20     2^-9      rho^2/2      dlt^4/24       -rho + rho^2                             rho^3 < 2^-60; expm1: < 2.4e-16 at the
//            (its two half-step stages: |dlt| < 2^-10, truncation < 8e-18 relative)                     guard's edge (1 ulp), 8e-18 at |dlt| = 1e-3
//   NARROW   2^-14     2^-7      rho^3/3      dlt^6/720      -rho + rho^2 - rho^3                     rho^4 < 2^-56; expm1: < 4.5e-17
//   WIDE     2^-11     2^-5      rho^4/4      dlt^8/40320    -rho + rho^2 - rho^3 + rho^4             rho^5 < 2^-55; expm1: < 2.4e-18
// (guard_ok holds exactly these bounds; no tier takes a Newton step.)  Beyond WIDE: the FULL tier, log / exp / reciprocal at
// every stage (struct Wave).
// Guard tracks the largest |rho| / |dlt| seen since it was last reset — through the HIGH WORD of each double read as
// a float: for |x| < 2^1017 that reading is finite and monotone in |x|, the thresholds are powers of two (exact in the
// high word), and two values fold into one v_max3_f32 with |.| as source modifiers (4 instructions per step instead
// of 8 v_max_f64).  |x| >= 2^1017, Inf and NaN read as float NaNs, which max ignores: NaN passes through as it always
// did (a dead trajectory stays on the fast path and ends in a non-finite SSq), and an increment that large can only
// come out of a state that is already beyond 1e150 — whose sum of squares rejects the proposal whichever path
// integrates it.  (Testing w for Inf at the end of the pair instead put five dependent instructions between the last
// result and the loop branch: +3 % at cfg1.)

struct Guard {
  float rho, dlt;
  float dlt_h;  // TIGHT: |dlt| of the two half-step stages, held to 2^-10 (truncation of their expm1 series < 8e-18)
  float rho_f;  // INSTEP: |c1| = |rho| / 2 of the full-step stage, held to 2^-21 — the same bound on rho (tight_incr_scaled)
  float del;    // INSTEP: |del| = |dlt| / k of the two half-step stages and of the full-step stage, held to Series::lim (tight_incr_scaled)
  float del_e;  // INSTEP: |del| of the step's end, held to Series::lim_e
  // INSTEP: a figure that comes once per step waits here for the next step's, and the two fold into their maximum with one
  // v_max3_f32 (guard_note): four instructions per step for the eight figures, as before the series was rescaled
  float p_rho, p_rho_f, p_del, p_del_e;
};

__device__ __forceinline__ float hi_as_float(double x) { return __builtin_bit_cast(float, __double2hiint(x)); }
constexpr float hi_pow2(int e) { return __builtin_bit_cast(float, (1023 + e) << 20); }  // high word of 2^e, as float


// leading series coefficients of a tier (kept in VGPRs, see Lane)
template <int T>
__device__ __forceinline__ void set_tier(Lane &L) {
  L.c_l1p = L.boa * (1.0 / 3.0);                                             // (TIGHT needs neither: Lane::nhboa)
  L.c_l1q = L.boa * (-1.0 / 4.0);                                            // (WIDE only)
  L.c_em1 = T == TIGHT ? 1.0 / 24.0 : (T == NARROW ? 1.0 / 720.0 : 1.0 / 40320.0);
  asm volatile("" : "+v"(L.c_l1p), "+v"(L.c_l1q), "+v"(L.c_em1));  // opaque: stays a register value, not re-materialised per step
}

template <int T>
__device__ __forceinline__ bool guard_ok(const Guard &g) {  // NaN passes through (see Guard)
  return (g.rho < (T == WIDE ? hi_pow2(-11) : (T == NARROW ? hi_pow2(-14) : hi_pow2(-20)))) &&
         (g.dlt < (T == TIGHT ? hi_pow2(-9) : (T == NARROW ? hi_pow2(-7) : hi_pow2(-5)))) && (T != TIGHT || g.dlt_h < hi_pow2(-10));
}

// Would the increments this trip measured also have fitted the next TIGHTER tier's guard, with a quarter to spare?  (The
// evidence a wave demotes itself on, struct Wave.)  Thresholds: 3/4 of tier T-1's bounds — 0.75 * 2^e has the high word
// of 1.5 * 2^(e-1).
constexpr float hi_pow2_34(int e) { return __builtin_bit_cast(float, ((1023 + e - 1) << 20) | 0x80000); }
template <int T>
__device__ __forceinline__ bool calm_enough(const Guard &g) {
  static_assert(T == NARROW || T == WIDE, "TIGHT has no tighter tier");
  return T == WIDE ? (g.rho < hi_pow2_34(-14) && g.dlt < hi_pow2_34(-7))
                   : (g.rho < hi_pow2_34(-20) && g.dlt < hi_pow2_34(-10));  // (TIGHT's half-step bound 2^-10 for every stage: stricter, simpler)
}

// ---------------------------------------------------------------------------------------------
// One classical RK4 step of size h; vl0/vlm/vl1 = V_l at t, t+h/2, t+h.
//
// Hot path (rk4_tight): the state carries (w, 1/th) at its own point, so stage 1 needs no
// transcendental at all; stages 2-4 and the step's end point are reached by tight_incr from the
// step's start point.  Straight-line code on purpose: with one wave per SIMD (cfg1) every
// instruction, nop and branch costs a full ~5-cycle issue slot (tools/microbench_fp64.hip).
// The largest increments of a PAIR of steps are checked once (integrate_pairs); if a lane left the tier's
// guard region (stiff small-Dc proposals) the pair is redone from the saved start point with full
// evaluations (rk4_cold).  Every kResync steps (w, 1/x) are recomputed in full so rounding in the
// incremental products cannot accumulate.
// ---------------------------------------------------------------------------------------------
constexpr int kResync = 512;  // power of two; every trip length below divides it.  (128 until round 3: 0.7 instructions per step.
                              // Four roundings per step on w make 5e-15 relative over 512 steps.)  Not at a chunk's first step: the
                              // state arrives there from a full evaluation or from the previous chunk's steps, never stale.
// The resync is the forward kernel's, the lockstep driver's and the NARROW / WIDE loops' of the sampler.  The sampler's in-step
// TIGHT trips (rk4_tight, INSTEP) have none: there (W, Rh) is a plain two-variable float64 recurrence and ms is not carried at
// all (rebuild_ms where somebody reads it).  The anchor injected more than it removed: only w was anchored (x is rebuilt from Rh),
// and to an ms ~ 6 Dc that one fma per step had rounded 512 times — each rounding, scaled by kia, 4e-15 in log w, against the
// 1e-16 of each of the four roundings the step puts on w itself.  Measured against the extended-precision RK4 (tests/test_ms_free.py:
// 2000 steps at h = 0.025 and 4000 at h = 0.0125, Dc 300 .. 5000, one and three parameters, damping on and off), largest relative
// error over the lanes, resynced form -> plain recurrence:  w 2.6e-13 .. 4.4e-13 -> 1.2e-14 .. 2.0e-14,  Rh 0.9e-14 .. 2.6e-14 ->
// 0.5e-14 .. 1.0e-14,  the sum of squares 0.5e-13 .. 2.6e-13 -> 1.5e-14 .. 2.8e-14.

// Both step functions return the weighted sum of the V derivatives, k1 + 2 k2 + 2 k3 + k4, IN UNITS OF vk (rhs_tail /
// rhs_tight): the velocity increment of the step is (h/6) vk = L.h6v times it.  V itself never feeds back into the RHS, so the hot loop does not carry it: with one
// step per output sample the acceleration (V_k - V_{k-1})/delta_t (RateStateModel.py:388) IS cacc * sum.
template <bool DAMP>
__device__ __forceinline__ double rk4_cold(State &s, double vl0, double vlm, double vl1, const Lane &L,
                                           const Consts &K) {
  double k0 = 0.0, k1 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma nounroll
  for (int st = 0; st < 4; ++st) {
    const double c = st == 0 ? 0.0 : (st == 3 ? K.h : K.hh);
    const double wgt = (st == 0 || st == 3) ? 1.0 : 2.0;
    const double vl = st == 0 ? vl0 : (st == 3 ? vl1 : vlm);
    const double x1 = __builtin_fma(c * L.vdc, k1, s.x);
    double w, rx, d0, d1, d2;
    eval_full(__builtin_fma(c, k0, s.ms), x1, L, K, w, rx);
    rhs_tail<DAMP>(w, rx, x1, vl, L, K, d0, d1, d2);
    s0 = __builtin_fma(wgt, d0, s0);
    s1 = __builtin_fma(wgt, d1, s1);
    s2 = __builtin_fma(wgt, d2, s2);
    k0 = d0;
    k1 = d1;
  }
  s.ms = __builtin_fma(K.h6, s0, s.ms);
  s.x = __builtin_fma(L.h6d, s1, s.x);
  return s2;
}

// The TIGHT tier's step.  s.rx holds Rh = (h/2Dc)/x (tier_enter), and every theta derivative of the step is carried
// SCALED by it, d1' = Rh (1 - w x): then rho of a half-step stage IS the previous stage's d1' (of the full-step stage
// twice it, of the step's end a third of the weighted sum), and with Rh x_0 = h/2Dc =: hhd the scaled derivative needs
// only constants and the previous d1':
//     Rh x_s = hhd + c_s d1'_prev  (c_s = hhd, hhd, hd),      d1' = Rh - w (Rh x_s),      (beta/x_s) d1 = bh (1 + q) d1',  bh = beta/hhd
//     (with damping W (Rh x_s / kvk), the constants hhdw = hhd/kvk, hdw = hd/kvk: rhs_tight),
// so neither rho = R d1 (four products per step) nor Rf, R6 and beta/x_0 (three per step) are formed: 5 instructions
// fewer than the unscaled form.  x itself is not carried at all: Rh IS the state (x = hhd / Rh where a full evaluation
// needs it), updated once per step, so Rh x_0 = hhd holds by construction.
//
// The wider tiers are the same step with longer series: NARROW one more term each — log1p to rho^3/3, expm1 to dlt^6/720,
// 1/x' = (1/x)(1 - rho + rho^2 - rho^3): |rho| < 2^-14, |dlt| < 2^-7 (truncations 4.5e-18, 4.5e-17, 1.4e-17), four
// instructions more per evaluation — and WIDE one and two more again — rho^4/4, dlt^8/40320, ... + rho^4: |rho| < 2^-11,
// |dlt| < 2^-5 (7e-18, 2.4e-18, 2.8e-17).  (Until round 3 they were an unscaled form with Newton steps on 1/x: 131 and 144
// instructions per step against 102 and 118, and their a-priori bounds reached less far down in Dc.)
template <int T, bool HALF>
__device__ __forceinline__ void tight_incr(double rho, double dk, const Lane &L, double w0, double &w, double &q, Guard &g) {
  g.rho = __builtin_fmaxf(g.rho, __builtin_fabsf(hi_as_float(rho)));
  double pb = L.nhboa;  // (b/a)(1 - rho/2 [+ rho^2/3 [- rho^3/4]])
  if (T == NARROW) pb = __builtin_fma(rho, L.c_l1p, pb);
  if (T == WIDE) pb = __builtin_fma(rho, __builtin_fma(rho, L.c_l1q, L.c_l1p), pb);
  const double dlt = __builtin_fma(-rho, __builtin_fma(rho, pb, L.boa), dk);
  // TIGHT: expm1 to dlt^4/24 at every stage, half-step stages held to |dlt| < 2^-10, the others to 2^-9
  if (T == TIGHT && HALF) g.dlt_h = __builtin_fmaxf(g.dlt_h, __builtin_fabsf(hi_as_float(dlt)));
  else g.dlt = __builtin_fmaxf(g.dlt, __builtin_fabsf(hi_as_float(dlt)));
  double e = L.c_em1;
  if (T == WIDE) {
    e = fm::hfma(e, dlt, 1.0 / 5040.0);
    e = fm::hfma(e, dlt, 1.0 / 720.0);
  }
  if (T != TIGHT) {
    e = fm::hfma(e, dlt, 1.0 / 120.0);
    e = fm::hfma(e, dlt, 1.0 / 24.0);
  }
  e = fm::hfma(e, dlt, 1.0 / 6.0);
  e = __builtin_fma(e, dlt, 0.5);
  e = __builtin_fma(e, dlt, 1.0);
  w = __builtin_fma(w0 * dlt, e, w0);
  const double r1 = __builtin_fma(rho, rho, -rho);                 // -rho + rho^2
  q = r1;                                                          // 1/x' = (1/x)(1 + q)
  if (T != TIGHT) q = __builtin_fma(-rho, q, -rho);                // NARROW: -rho + rho^2 - rho^3
  if (T == WIDE) q = __builtin_fma(-rho, q, -rho);                 // WIDE: ... + rho^4
}

// The in-step mode's increments (TIGHT trips of the sampler: rk4_tight, INSTEP), with the stage stiffness folded into the series.
// Write k for the factor that puts a stage's ms derivative d into increment units: khh at the half-step stages, kh at the
// full-step stage, kh6 at the step's end.  dlt = k d - rho (b/a)(1 - rho/2) is never formed; the step works on del = dlt / k,
//     del = d - rho (B + N rho),   B = (b/a)/k,  N = -(b/2a)/k        (two fmas on d as it stands: the product k d is gone),
// and the series takes k into its coefficients: w' = w0 + (w0 del) Ek(del) with
//     Ek(del) = k E(k del) = k + (k^2/2) del + (k^3/6) del^2 (+ (k^4/24) del^3)
// — the Horner depth of E, its leading 1 now the k that the lane holds anyway: one operation fewer per increment, four per step.
// k del is the same number as dlt, so every truncation bound above holds as it stands.  Of the roundings, the one of k d has
// moved into the constants (each within 2 ulp, on terms below the leading one); d0 = V_l - v reaches del as it left the stage,
// so nothing is rounded in front of that cancellation (pre-scaling d0 would do just that).
//   half-step stages  r = rho, the previous stage's d1'; the series to del^2: their w is a stage value, not the carried state — at
//                     the stage guard's edge, |dlt| = 2^-10, the dropped dlt^4/24 is 3.8e-14 of it, which reaches the step's sample
//                     with weight 1/3 and the carried state through another factor |dlt|; at Dc ~ 1000 (|dlt| ~ 1e-4) it is 4e-18;
//   full-step stage   r = c1 = rho / 2, the previous stage's d1' as it stands: (b/a) log1p(2 c1) / kh = c1 (B - B c1) with the
//                     half-step stages' B = (b/a)/khh, and the sum c1 + c1 is never formed;
//   step's end        r = t1 = 3 rho, the weighted sum as it stands: (b/a) log1p(t1/3) / kh6 = t1 (B - (B/6) t1), the same B again.
// The stage brackets take 1/(1 + rho) to FIRST order: brx = bh (1 - rho), one fma on the previous d1' at the half-step stages
// (rk4_tight) and on c1 at the full-step stage (Lane::bh2) — no q there.  A stage's brx only forms g = d0 - brx d1', which
// feeds the stage's dV/dt (the sample, cv sum wgt W g) and, with damping, d0 -= W g with W = k1 V_ref w / a ~ 1e-5; V never
// feeds back.  So the dropped bh rho^2 d1' reaches the sample as it stands, the state scaled down by W, and is not carried
// from step to step: |delta g| <= |bh| rho^2 |d1'| per stage, and the d1' of a half-step stage is the next stage's rho (or c1),
// so <= |bh| lim^3 under a limit lim on |rho| (the full-step stage's own d1' is held through the step's end, t1 = 3 rho: it
// stays within 7 lim whatever the others do, and is one of them to a part in 1e3 on any smooth trajectory).
// The guard holds |bh| lim^3 to 2^-47 V_ref by a per-lane limit on |rho| (Series::lim_rho: it binds before 2^-20 where |bh| >
// 8192 V_ref) — under the dlt^4/24 above; at Dc ~ 1000, h = 0.025 the term is 1e-18.  The step's end keeps its
// q = -rho + rho^2: that one updates the carried Rh.
// The log1p bracket pb = B + N rho is formed ONCE for the two half-step stages, at the first one's rho_a = a1; the second takes it
// with its own r = rho_b = b1, del = d - rho_b (B + N rho_a): one fma fewer per step, 67 operations.  What that leaves out of the
// second stage's dlt is k rho_b N (rho_b - rho_a) = (b/2a) |rho_b| |rho_b - rho_a|, and from rhs_tight
//     rho_b - rho_a = (Rh - w_b xh (1 + a1)) - (Rh - W xh) = -W xh (expm1(dlt_a) + (1 + expm1(dlt_a)) a1),   |W xh| = |Rh - rho_a| <= |Rh| + |rho|,
// so |rho_b - rho_a| <= (|Rh| + |rho|)(|dlt| + |rho|) to first order: second order in a second-order term.  Under the guard |dlt| < 2^-10
// at that stage and |rho| < 2^-20.  Rh drifts by a factor 1 + q per step, |q| < 2^-19: under 1 % in the few thousand steps of a chunk,
// so with Rh0 the state's where a Series was formed |Rh| + |rho| <= 1.01 |Rh0| + 2^-20 <= 2 |Rh0| wherever |Rh0| >= 1.02 * 2^-20; below
// that the term is under (b/a) 2^-49 whatever the limit.  The limit
//     |rho| < lim_pb = 2^-43 / ((b/2a) (2^-10 + 2^-20) 2 |Rh0|)                                       (tight_pb_limit, rounded down)
// holds the term to 2^-43 = 1.1e-13 in dlt — a stage value's, like the dlt^4/24 = 3.8e-14 the half-step stages drop at the same
// edge; it joins Series::lim_rho, lim_c1 and bmax through a min with tight_rho_limit's and costs a trip nothing.  It binds before
// 2^-20 where (b/a) |Rh| > 1.22e-4: with the default (a, b) below TIGHT's a-priori edge; at Dc ~ 1000, h = 0.025 it is 8 * 2^-20.
// The FULL-step stage does not take the shared bracket: its rho is 2 c1, TWICE a half-step stage's, so rho_s - rho_a ~ rho_a there and
// B + N a1 in place of B - B c1 would leave out (b/a) |c1| |2 c1 - a1| ~ (b/a) c1^2 — half of the second-order term outright, 2.3e-13
// in dlt at 0.9 of the guard's edge, which no limit on |Rh| mends (the limit on |rho| it would take is near 0.3 * 2^-20).
// The guard (GUARD; without it the same arithmetic, instruction for instruction, for a trip whose start state proves that no
// increment can reach a threshold: tight_needs_guard) holds del to the regions of dlt: |del| < 2^-10 / |khh| at the half-step
// stages — which is 2^-9 / |kh|, so the full-step stage shares the figure — and < 2^-9 / |kh6| at the step's end; rho and c1 as ever.
// The thresholds are per lane and rounded DOWN: a trip earlier, never later.
struct Series {
  double B, N, N6;     // (b/a)/khh, -B/2, -B/6
  double h1, h2;       // half-step stages: khh^2/2, khh^3/6
  double f1, f2, f3;   // full-step stage: kh^2/2, kh^3/6, kh^4/24
  double e1, e2, e3;   // step's end: kh6^2/2, kh6^3/6, kh6^4/24
  float lim, lim_e;    // the guard's thresholds on |del|: high words, read as floats (struct Guard)
  float lim_rho, lim_c1;  // the guard's thresholds on |rho| and on |c1|, half of it (tight_rho_limit), high words as well
  float bmax;          // the unguarded loop's: what tight_needs_guard holds its bound on |d1'| to, 0.9 lim_rho / 2
};

// The lane's limit on |rho| in the in-step TIGHT step: min(2^-20, cbrt(2^-47 V_ref / |bh|)), rounded DOWN — the first from the
// series in rho as ever, the second holds the rho^2 term that the stage brackets leave out to 2^-47 V_ref (tight_incr_scaled).
// The cube root as y^(-1/3) of y = 2^47 |bh| / V_ref: a seed from the exponent (a third of the high word taken from a
// constant: within 10.3 % in y r^3) and two Newton steps r <- r (4 - y r^3) / 3, each of which lands BELOW the root (by 2/9 of
// the square of that figure: -2.5e-3, then -1.2e-5); the factor 1 - 2^-30 covers the roundings.  bh = 0 gives a huge r and
// the first limit, a NaN anywhere the same (fmin keeps 2^-20: the path as it was), an infinite bh a limit of -inf, which every
// compare fails.  A dozen and a half operations, where a Series is formed and once per solve (wave_begin): 0.0003 per step at
// nsteps 2000.
__device__ __forceinline__ double tight_rho_limit(double bh, const Consts &K) {
  const double y = (0x1.0p47 * K.inv_vref) * __builtin_fabs(bh);
  double r = __hiloint2double((int)(0x553ee800u - (unsigned)__double2hiint(y) / 3u), 0);
#pragma unroll
  for (int it = 0; it < 2; ++it) r = (r * (1.0 / 3.0)) * __builtin_fma(-(y * r), r * r, 4.0);
  return __builtin_fmin(0x1.0p-20, (1.0 - 0x1.0p-30) * r);
}
// What the a-priori bound holds every |d1'| of a trip to, given the lane's limit on rho: 0.9 of the limit on c1 (tight_needs_guard
// through Series::bmax, which keeps the high word — once more rounded down, by 2^-20 of the figure at most; W.never as it stands).
__device__ __forceinline__ double tight_bmax(double lim_rho) { return 0.45 * lim_rho; }
// The lane's limit on |rho| that holds what the shared half-step bracket leaves out to 2^-43 (tight_incr_scaled):
//     lim_pb = 2^-43 / ((b/2a) (2^-10 + 2^-20) 2 |Rh|) = (2^-33 / (1 + 2^-10)) / |(b/a) Rh|,   rounded DOWN:
// the constant is the double below the quotient, the factor 1 - 2^-30 covers the product's rounding and the reciprocal's ulp, and
// the high word that the guard keeps rounds down once more.  Rh is the state's where a Series is formed (make_series).  (b/a) Rh = 0
// gives a NaN (fm::rcp), and so does a NaN in either factor: the fmin at the caller keeps its other operand, the limit as it was
// (as tight_rho_limit treats them); an infinite product the same (fm::rcp's Newton step on the seed 0 forms inf * 0): such a state is
// already lost, and its rho trips the limit as it was.  Eight operations per Series.
__device__ __forceinline__ double tight_pb_limit(double boa, double Rh) {
  constexpr double C = 0x1.ff801ff801ff8p-34;  // 2^-33 / (1 + 2^-10) = 2^-34 * 1.99805..., truncated
  return ((1.0 - 0x1.0p-30) * C) * fm::rcp(__builtin_fabs(boa * Rh));
}
// Formed where a loop of in-step trips is entered (integrate_multi), from a value the compiler cannot trace back (local_value):
// held from make_lane on, the constants were live through every other tier's loop as well and the sampler kernels spilled
// (44 to 88 bytes of scratch per lane).  Fifty-odd operations per entry; at the headline shape a solve enters twice or so.
// Rh: the state's at the entry, for the limit that goes with the shared half-step bracket (tight_pb_limit).
template <bool GUARD>
__device__ __forceinline__ Series make_series(const Lane &L, const Consts &K, double Rh) {
  Series S;
  const double khh = local_value(L.khh);
  const double ik = fm::rcp(khh);
  S.B = L.boa * ik;
  S.N = -0.5 * S.B;
  S.N6 = S.B * (-1.0 / 6.0);
  const double kh = khh + khh, kh6 = khh * (1.0 / 3.0);  // (Lane::kh to the bit; Lane::kh6 to an ulp)
  const double k2 = khh * khh, f2 = kh * kh, e2 = kh6 * kh6;
  S.h1 = 0.5 * k2;
  S.h2 = (k2 * khh) * (1.0 / 6.0);
  S.f1 = 0.5 * f2;
  S.f2 = (f2 * kh) * (1.0 / 6.0);
  S.f3 = (f2 * f2) * (1.0 / 24.0);
  S.e1 = 0.5 * e2;
  S.e2 = (e2 * kh6) * (1.0 / 6.0);
  S.e3 = (e2 * e2) * (1.0 / 24.0);
  S.lim = S.lim_e = S.lim_rho = S.lim_c1 = 0.0f;
  // (formed here, like the rest: see above; fmin keeps the first limit where the second is a NaN)
  const double lim_rho = __builtin_fmin(tight_rho_limit(local_value(L.bh), K), tight_pb_limit(L.boa, Rh));
  S.bmax = hi_as_float(tight_bmax(lim_rho));  // (the high word of 0.9 * 2^-21 where the first limit holds)
  if constexpr (GUARD) {
    S.lim_rho = hi_as_float(lim_rho);
    S.lim_c1 = hi_as_float(0.5 * lim_rho);
    // 2^-10 / |khh| and 3 * 2^-9 / |khh|.  The factor 1 - 2^-30 covers the ulps of the reciprocal and of kh6 against khh / 3;
    // keeping the high word alone rounds down once more (at most 2^-20 of the threshold in all).
    const double aik = (1.0 - 0x1.0p-30) * __builtin_fabs(ik);
    S.lim = hi_as_float(0x1.0p-10 * aik);
    S.lim_e = hi_as_float(0x1.8p-8 * aik);
  }
  return S;
}

// The bracket of a stage's own r: B + N rho with rho = r at a half-step stage, 2 r at the full-step stage, r / 3 at the step's end.
template <int STAGE>
__device__ __forceinline__ double tight_bracket(double r, const Series &S) {
  return STAGE == 0 ? __builtin_fma(r, S.N, S.B) : (STAGE == 1 ? __builtin_fma(-r, S.B, S.B) : __builtin_fma(r, S.N6, S.B));
}

// a figure that comes once per step: held on even steps, folded with the next step's on odd ones (struct Guard)
__device__ __forceinline__ void guard_note(float &acc, float &pend, double x, bool odd) {
  const float ax = __builtin_fabsf(hi_as_float(x));
  if (odd) acc = __builtin_fmaxf(__builtin_fmaxf(acc, pend), ax);
  else pend = ax;
}

// STAGE 0: a half-step stage, q left alone (the caller's bracket is bh - bh rho);  1: the full-step stage, q = brx = bh - 2 bh c1;
// 2: the step's end, q = -rho + rho^2 of rho = t1/3.
// odd: the step's parity within its trip (guard_note).
// pb: the bracket B + N rho of the stage — its own (tight_bracket) or, at the second half-step stage, the first one's (rk4_tight).
template <int STAGE, bool GUARD>
__device__ __forceinline__ void tight_incr_scaled(double r, double pb, double d, const Lane &L, const Series &S, double w0, double &w, double &q,
                                                  Guard &g, bool odd) {
  const double del = __builtin_fma(-r, pb, d);
  double e;
  if constexpr (STAGE == 0) e = __builtin_fma(__builtin_fma(S.h2, del, S.h1), del, L.khh);
  else if constexpr (STAGE == 1) e = __builtin_fma(__builtin_fma(fm::hfma(S.f3, del, S.f2), del, S.f1), del, L.kh);
  else e = __builtin_fma(__builtin_fma(fm::hfma(S.e3, del, S.e2), del, S.e1), del, L.kh6);
  w = __builtin_fma(w0 * del, e, w0);
  if constexpr (STAGE == 1) {
    q = __builtin_fma(r, L.bh2, L.bh);
    if constexpr (GUARD) {
      guard_note(g.rho_f, g.p_rho_f, r, odd);
      guard_note(g.del, g.p_del, del, odd);
    }
  } else {
    const double rho = STAGE == 0 ? r : r * (1.0 / 3.0);  // the step's end: (h/6Dc)/x times the unscaled sum
    if constexpr (STAGE == 2) q = __builtin_fma(rho, rho, -rho);
    if constexpr (GUARD && STAGE == 0) {  // two of each per step: they fold within the step
      g.rho = __builtin_fmaxf(g.rho, __builtin_fabsf(hi_as_float(rho)));
      g.del = __builtin_fmaxf(g.del, __builtin_fabsf(hi_as_float(del)));
    }
    if constexpr (GUARD && STAGE == 2) {
      guard_note(g.rho, g.p_rho, rho, odd);
      guard_note(g.del_e, g.p_del_e, del, odd);
    }
  }
}

// d0 = V_l - V_ref w,  d1' = Rh - w xr  (xr = Rh x at the stage),  g = d0 - brx d1'  (brx = bh (1 + q); in the in-step mode
// bh (1 - rho): tight_incr_scaled) and the damping pass.
// g is the bracket of dV/dt = vk w g, one fma on the two derivatives the stage forms anyway.  With damping `w` is W = kvk w
// (Lane::vrw; vr = V_ref/kvk, xr scaled by 1/kvk with it), so the pass d0 -= (kvk w) g, g -= (kvk w) g takes no product; the
// caller forms W g (the stage's dV/dt in units of vk/kvk) inside its weighted sum.  (Rounds 1-2 wrote g linear in w so that all but one fma
// was ready before w — the end of the previous stage's dependency chain — arrived: one instruction more per stage for one
// dependent level less; measured in round 3, profiles/r03/ab_gform.log, the shorter stream wins at every shape.)
template <bool DAMP>
__device__ __forceinline__ void rhs_tight(double w, double xr, double Rh, double vl, double brx, double vr, double &d0, double &d1,
                                          double &g) {
  d1 = __builtin_fma(-w, xr, Rh);
  d0 = __builtin_fma(-vr, w, vl);
  g = __builtin_fma(-brx, d1, d0);
  if (DAMP) {
    d0 = __builtin_fma(-w, g, d0);
    g = __builtin_fma(-w, g, g);
  }
}

//
// INSTEP (TIGHT trips of the sampler, one step per sample: integrate_multi): the step adds its sample's squared residual to
// *ssq itself (`first`: starts that sum), r = cv sv + (2 cv sm - obs), and returns nothing of use — no per-step sample leaves the step, so a trip keeps
// neither its samples nor, beyond each step, its observations in registers.  Its half-step stages take the expm1 series
// one term shorter and its full-step stage the half increment, all four increments in units of their stage's stiffness (tight_incr_scaled;
// S: the series constants, odd: the step's parity in its trip, for the guard).
template <bool DAMP, int T, bool INSTEP = false, bool GUARD = true>
__device__ __forceinline__ double rk4_tight(State &s, double vl0, double vlm, double vl1, const Lane &L, const Consts &K, Guard &g,
                                            double obs = 0.0, double *ssq = nullptr, bool first = false, const Series *S = nullptr,
                                            bool odd = false) {
  static_assert(!INSTEP || T == TIGHT, "the in-step sum of squares is the TIGHT step's");
  static_assert(GUARD || INSTEP, "the unguarded step is the in-step mode's");
  double a0, a1, a2, b0, b1, b2, c0, c1, c2, e0, e1, e2, w, q = 0.0;
  const double Rh = s.rx;
  const double vr = L.vrw, xh = L.hhdw, xf = L.hdw;  // (V_ref, hhd, hd) / kvk with damping: s.w is W (Lane::vrw)
  rhs_tight<DAMP>(s.w, xh, Rh, vl0, L.bh, vr, a0, a1, a2);
  double sv = s.w * a2;  // k1 + k4 of dV/dt (in units of vk, vk/kvk with damping), and k2 + k3 below: 5 instructions for the weighted sum
  double pb = 0.0;  // INSTEP: the first half-step stage's bracket, which the second one takes as well (tight_incr_scaled)
  if constexpr (INSTEP) {
    pb = tight_bracket<0>(a1, *S);
    tight_incr_scaled<0, GUARD>(a1, pb, a0, L, *S, s.w, w, q, g, odd);
  } else tight_incr<T, true>(a1, L.khh * a0, L, s.w, w, q, g);
  rhs_tight<DAMP>(w, __builtin_fma(xh, a1, xh), Rh, vlm, INSTEP ? __builtin_fma(-L.bh, a1, L.bh) : __builtin_fma(L.bh, q, L.bh), vr, b0, b1, b2);
  double sm = w * b2;
  if constexpr (INSTEP) tight_incr_scaled<0, GUARD>(b1, pb, b0, L, *S, s.w, w, q, g, odd);
  else tight_incr<T, true>(b1, L.khh * b0, L, s.w, w, q, g);
  rhs_tight<DAMP>(w, __builtin_fma(xh, b1, xh), Rh, vlm, INSTEP ? __builtin_fma(-L.bh, b1, L.bh) : __builtin_fma(L.bh, q, L.bh), vr, c0, c1, c2);
  sm = __builtin_fma(w, c2, sm);
  if constexpr (INSTEP) {
    double brx;
    tight_incr_scaled<1, GUARD>(c1, tight_bracket<1>(c1, *S), c0, L, *S, s.w, w, brx, g, odd);
    rhs_tight<DAMP>(w, __builtin_fma(xf, c1, xh), Rh, vl1, brx, vr, e0, e1, e2);
  } else {
    tight_incr<T, false>(c1 + c1, L.kh * c0, L, s.w, w, q, g);
    rhs_tight<DAMP>(w, __builtin_fma(xf, c1, xh), Rh, vl1, __builtin_fma(L.bh, q, L.bh), vr, e0, e1, e2);
  }
  sv = __builtin_fma(w, e2, sv);
  const double t0 = a0 + 2.0 * b0 + 2.0 * c0 + e0;
  const double t1 = a1 + 2.0 * b1 + 2.0 * c1 + e1;
  if constexpr (INSTEP) {
    tight_incr_scaled<2, GUARD>(t1, tight_bracket<2>(t1, *S), t0, L, *S, s.w, w, q, g, odd);
  } else {
    const double rho = t1 * (1.0 / 3.0);  // (h/6Dc)/x times the unscaled sum
    tight_incr<T, false>(rho, L.kh6 * t0, L, s.w, w, q, g);
  }
  if constexpr (!INSTEP) s.ms = __builtin_fma(K.h6, t0, s.ms);  // (the in-step trips leave ms behind: rebuild_ms)
  s.w = w;
  s.rx = __builtin_fma(Rh, q, Rh);  // x' = x (1 + rho), exact to rounding for |rho| < 2^-20; like w, resynced
  if constexpr (INSTEP) {
    const double r = __builtin_fma(sv, L.cv, __builtin_fma(sm, L.cv2, -obs));
    *ssq = first ? r * r : __builtin_fma(r, r, *ssq);
    return 0.0;
  }
  return __builtin_fma(2.0, sm, sv);
}

// STIFF: make_lane's; ikappa = 1 / (k Dc) stands for the reciprocal of the coupling's literal
template <bool STIFF = false>
__device__ __forceinline__ State initial_state(double dc, const Lane &L, const Consts &K, double ikappa = 0.0) {
  State s;
  if constexpr (STIFF) s.ms = (K.mu0 * dc) * ikappa;
  else s.ms = (K.mu0 * dc) * (1.0 / (1e-2 * 10));  // mu(0)/k' = mu_t_zero/k', RateStateModel.py:367-377
  s.x = K.V_ref * ((dc * K.inv_vref) * L.inv_dc);  // V_ref theta(0)/Dc with theta(0) = Dc/V_ref: 1 to rounding
  s.V = K.V_ref;
  eval_full(s.ms, s.x, L, K, s.w, s.rx);
  return s;
}

// ---------------------------------------------------------------------------------------------
// LDS staging.  Chunk c covers output samples k0 .. k0+kn-1 (k0 = 1 + c*kc): it needs
// 2*S*kn+1 loading values and kn observations.  Layout: [ vl : 2*S*kc+1 ][ data : kc ][ data_0 ] — the last word holds the
// observation's sample 0, which belongs to no chunk (acc[0] = 0, RateStateModel.py:371: its square starts every sum of
// squares).  Until round 4 every forward solve read it from global memory and waited for it: a cache round trip per
// proposal, and — vector loads and stores retire in order on one counter — a wait for the trace row the previous iteration
// had just stored.  With it staged here the sampler's iteration loop holds no vector load at all.
// Every thread of the workgroup must call stage_chunk (it contains the barriers).
// ---------------------------------------------------------------------------------------------
constexpr int kLdsPad = 0;
__device__ __forceinline__ int lds_data_offset(const Consts &K) { return 2 * K.S * K.kc + 1 + kLdsPad; }
__device__ __forceinline__ int lds_d0_offset(const Consts &K) { return lds_data_offset(K) + K.kc; }

__device__ __forceinline__ void stage_chunk(double *lds, const Consts &K, int k0, int kn) {
  const int nv = 2 * K.S * kn + 1;
  const int base = 2 * K.S * (k0 - 1);
  __syncthreads();  // every wave is done with the previous chunk
  for (int i = threadIdx.x; i < nv; i += blockDim.x) lds[i] = K.vl[base + i];
  if (K.data) {
    double *ld = lds + lds_data_offset(K);
    for (int i = threadIdx.x; i < kn; i += blockDim.x) ld[i] = K.data[k0 + i];
    if (threadIdx.x == 0) lds[lds_d0_offset(K)] = K.data[0];
  }
  __syncthreads();
}

// Output bookkeeping of a chunk.  S1: one step per output sample (the BASELINE configs), every step of a trip emits a
// sample; otherwise a sample is emitted every K.S steps (wave-uniform phase counter).
struct Emit {            // output bookkeeping of a chunk
  int ko;                // next output sample of the chunk (0 .. kn-1)
  int phase;             // RK4 steps since the last emitted sample (S > 1 only)
  double vprev;          // V at the last emitted sample
};

// acceleration sample ko of the chunk from the velocities at its two ends (RateStateModel.py:388) + SSq term;
// `obs` is the observation at that sample (read from LDS by the caller, early, so its latency is hidden)
template <bool WANT_SSQ, bool WANT_ACC>
__device__ __forceinline__ void emit_at(double vnow, double vprev, int ko, double obs, const Consts &K, int k0,
                                        double &ssq, bool active, double *acc_out, int64_t stride) {
  const double ak = (vnow - vprev) * K.inv_dt;
  if (WANT_ACC && active) acc_out[(int64_t)(k0 + ko) * stride] = ak;
  if (WANT_SSQ) {
    const double r = ak - obs;
    ssq = __builtin_fma(r, r, ssq);
  }
}

// the same sample straight from the step's derivative sum (one step per output sample): ak = cacc vk * dvs
template <bool WANT_SSQ, bool WANT_ACC>
__device__ __forceinline__ void emit_incr(double dvs, int ko, double obs, const Lane &L, int k0, double &ssq,
                                          bool active, double *acc_out, int64_t stride) {
  if (WANT_ACC && active) acc_out[(int64_t)(k0 + ko) * stride] = dvs * L.cv;
  if (WANT_SSQ) {
    const double r = __builtin_fma(dvs, L.cv, -obs);  // one rounding; identical with and without WANT_ACC
    ssq = __builtin_fma(r, r, ssq);
  }
}

template <bool WANT_SSQ, bool WANT_ACC>
__device__ __forceinline__ void emit_sample(double vnow, Emit &em, double obs, const Consts &K, int k0, double &ssq,
                                            bool active, double *acc_out, int64_t stride) {
  emit_at<WANT_SSQ, WANT_ACC>(vnow, em.vprev, em.ko, obs, K, k0, ssq, active, acc_out, stride);
  em.vprev = vnow;
  ++em.ko;
}

// One trip: NU straight-line steps of tier T from s (L already carries the tier's coefficients, set_tier);
// dv[j] = the weighted V-derivative sum of step j.  Returns whether this lane left the tier's guard region — its
// values are then not to be used: the caller restores the state it saved and takes trip_cold.
template <bool DAMP, int T, int NU>
__device__ __forceinline__ bool trip_fast(const double *v, const Lane &L, const Consts &K, State &s, double (&dv)[NU], bool *calm = nullptr) {
  Guard g = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < NU; ++j) dv[j] = rk4_tight<DAMP, T>(s, v[2 * j], v[2 * j + 1], v[2 * j + 2], L, K, g);
  if constexpr (T != TIGHT) {
    if (calm) *calm = calm_enough<T>(g);
  }
  return !guard_ok<T>(g);
}

// the same trip with a full evaluation at every stage (exact whatever the increments), (w, 1/x) re-formed at its end in
// tier T's representation
template <bool DAMP, int T, int NU>
__device__ __forceinline__ void trip_cold(const double *v, const Lane &L, const Consts &K, State &s, double (&dv)[NU]) {
  tier_x<T>(s, L);
#pragma unroll 1
  for (int j = 0; j < NU; ++j) {  // one copy of the cold step; its result goes to dv[j] by selects, so that dv stays in registers
    const double r = rk4_cold<DAMP>(s, v[2 * j], v[2 * j + 1], v[2 * j + 2], L, K);
#pragma unroll
    for (int m = 0; m < NU; ++m) dv[m] = m == j ? r : dv[m];
  }
  eval_full_t<DAMP, T>(s, L, K);
}

// the cold trip of the in-step mode (one step per sample, the sum of squares alone): each cold step's sample goes straight into
// ssq against its observation ob[j], in emit_incr's arithmetic — no dv[] here either
template <bool DAMP, int T, int NU>
__device__ __forceinline__ void trip_cold_ssq(const double *v, const double *ob, const Lane &L, const Consts &K, State &s, double &ssq) {
  tier_x<T>(s, L);
#pragma unroll 1
  for (int j = 0; j < NU; ++j) {
    const double dvs = rk4_cold<DAMP>(s, v[2 * j], v[2 * j + 1], v[2 * j + 2], L, K);
    emit_incr<true, false>(dvs, j, ob[j], L, 0, ssq, false, nullptr, 0);
  }
  eval_full_t<DAMP, T>(s, L, K);
}

// the same for a caller that holds the PLAIN state between trips — (ms, x) with rx = 1 / x, as the init kernels do: cold steps
// straight from (ms, x), then (w, 1/x) re-evaluated at the trip's end point
template <bool DAMP, int NU>
__device__ __forceinline__ void trip_cold_plain(const double *v, const Lane &L, const Consts &K, State &s, double (&dv)[NU]) {
#pragma unroll 1
  for (int j = 0; j < NU; ++j) {  // one copy of the cold step; its result goes to dv[j] by selects, so that dv stays in registers
    const double r = rk4_cold<DAMP>(s, v[2 * j], v[2 * j + 1], v[2 * j + 2], L, K);
#pragma unroll
    for (int m = 0; m < NU; ++m) dv[m] = m == j ? r : dv[m];
  }
  eval_full(s.ms, s.x, L, K, s.w, s.rx);
}

// ---------------------------------------------------------------------------------------------
// Wave-level control of one forward solve.  Every member is wave-uniform (ballots, step counts), i.e. lives in SGPRs.
//
// alive    lanes whose result can still matter: in bounds (the caller's activity mask) and not yet CERTAINLY REJECTED.
//          The sum of squares is a sum of non-negative terms, so its partial sums only grow, and the accept test
//          (MCMC.py:327-331) is monotone in SSq: once a lane's running sum exceeds `thr` — the caller's conservative bound
//          on the largest SSq that could still be accepted with this iteration's uniform — the proposal is rejected
//          whatever the rest of the series adds.  Such a lane stops counting: its guard trips are ignored, it no longer
//          holds its wave in a wider tier, and a wave with no lane left ends the solve.  Nothing observable changes: a
//          rejected proposal leaves the chain where it was, and its SSq is never stored.
// need[]   need[T-1] = lanes that cannot run a tier tighter than T (T = NARROW, WIDE, FULL): the a-priori bound of the lane's
//          mu increment (|V_l - v| <~ 1.2 V_ref against the tiers' |dlt| guards), escalated when the lane's guard trips.
//          The wave's tier is the widest one an ALIVE lane needs, re-decided whenever that set changes — so a stiff
//          small-Dc proposal costs its wave the wider tier only until its sum of squares has disqualified it.
// FULL     the full-evaluation tier (log / exp / reciprocal at every stage, exact whatever the increments): entered by a lane
//          whose WIDE guard trips, left again after kFullRetry steps to try WIDE once more (`stiff` lanes, whose a-priori
//          bound is beyond 2^-3, stay).  Until round 4 a tripped WIDE trip was redone cold and the next trip tried the
//          fast step again: a wave with one stiff lane paid fast + cold on every trip.
// calm     demotion on evidence.  The a-priori classes are BOUNDS (|V_l - v| <~ 1.2 V_ref), and the loading oscillation that
//          drives the increments decays like exp(-t/20): a lane that needs WIDE for its first forty steps is fine in NARROW for
//          the other four hundred.  Every trip measures its largest increments anyway (Guard); when, for kCalmSteps steps
//          in a row (two periods of the oscillation at h = 0.1), every alive lane's would also have fitted the next tighter
//          tier's guard with a quarter to spare, the wave's alive lanes move one tier tighter.  If that turns out wrong the
//          ordinary escalation takes the lane back (one cold trip) — rare, because the evidence is the increments themselves.
// ---------------------------------------------------------------------------------------------
constexpr int kFullRetry = 32;
constexpr int kCalmSteps = 16;  // steps of evidence before a wave demotes itself one tier (>= two loading periods at h = 0.1)
struct Wave {
  unsigned long long alive;
  unsigned long long need[3];
  unsigned long long stiff;
  int next_resync;   // chunk-local step at which (w, Rh) are next re-evaluated in full (kResync)
  int full_run;      // steps since the FULL tier was (re-)entered
  int calm;          // consecutive steps in which every alive lane's increments would have fitted the next tighter tier
  // statistics of this solve (rsf_mcmc_counters): wave-steps per tier, wave-steps of fast trips thrown away by a tripped
  // guard, and the sum over steps of the number of alive lanes (lane utilisation = lane_steps / (64 * all steps))
  uint32_t steps[4], redone, lane_steps;
  // Consts::vl_lo / vl_hi as scalars of their own (wave_begin), for tight_needs_guard.  Read from K at every trip they kept the
  // 16-dword kernel-argument tuple that holds them live through the TIGHT loop: the compiler spilled the tuple and reloaded 16
  // scalars per trip (22 lane moves in the loop; 6 with the copies).
  double vl_lo, vl_hi;
  // lanes that tight_needs_guard cannot be expected to free at any trip of this solve (wave_begin): while one of them is alive the
  // wave does not evaluate the bound at all.  At one wave per SIMD a trip waits out the bound's whole dependency chain and the
  // branch on it: +1.9 % at configs[1] (h = 0.1, Dc ~ 1000: the bound never holds there), nothing with this mask.
  unsigned long long never;
  bool guard_next;  // the bound just failed at this trip: one guarded trip before it is asked again (integrate_multi, UNGUARD)
  uint32_t unguarded;  // the wave-steps among steps[TIGHT] whose trip ran without the guard (tight_needs_guard)
  // s.ms is stale: in-step TIGHT trips have run since it was last formed (they do not carry it: rk4_tight, INSTEP).  Set by the
  // in-step loops of integrate_multi; whoever is about to read ms forms it from (W, Rh) first (rebuild_ms) and clears this.
  bool ms_stale;
};

// the constants of tight_needs_guard, for trips of NU steps
template <int NU>
struct TightBound {
  static constexpr double R = 0x1.0p-20, B = 0x1.0p-21, Dmax = 0.9 * 0x1.0p-9, gm1 = 1.02 * NU * Dmax;
  static constexpr double G = 1.02 * NU, kap = (NU + 1) * R;  // (the limit on rb is the lane's: Series::bmax)
  static_assert(NU * Dmax < 0.035, "exp(x) - 1 <= 1.02 x needs x < 0.035");
};

__device__ __forceinline__ unsigned long long ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool lane_in(unsigned long long mask) { return (mask >> (threadIdx.x & 63)) & 1; }
// a double from the lane that DPP control CTRL names (quad_perm, row_half_mirror, ...): two moves in the VALU, one per half —
// no trip through the LDS pipe as a general shuffle (ds_bpermute) takes
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// (the statistics members are the caller's to zero: they accumulate over the solves of a launch)
// NU: steps per whole TIGHT trip of the solve (W.never)
template <int NU>
__device__ __forceinline__ void wave_begin(Wave &W, bool active, const Lane &L, const Consts &K) {
  const double dk = 1.2 * K.V_ref * K.h * L.kia;
  // W.never: what tight_needs_guard's two figures are AT LEAST, whatever the state — |V_l - v| ranges over half the table's range
  // or more, and Rh0 = hhd / x — taken at x = 1, the steady state at V_ref.  (A gate on speed alone: a lane it names keeps the
  // guard, which is always right; a lane it misses fails the bound itself.)  The limit on rmin is the lane's, as tight_needs_guard's
  // (tight_bmax; not truncated to its high word here: rb >= rmin, so the stricter of the two figures is the one that decides).
  using TB = TightBound<NU>;
  const double dmin = __builtin_fma(__builtin_fabs(L.kh), 0.5 * (K.vl_hi - K.vl_lo), __builtin_fabs(L.boa) * TB::R);
  const double rmin = __builtin_fabs(L.hhd) * __builtin_fma(dmin, TB::G, TB::kap);
  W.never = ballot(active && !(dmin < TB::Dmax && rmin < tight_bmax(tight_rho_limit(L.bh, K))));
  W.guard_next = false;
  W.ms_stale = false;
  W.alive = ballot(active);
  W.need[0] = ballot(active && !(dk < 0x1.0p-9));
  W.need[1] = ballot(active && !(dk < 0x1.0p-7));
  W.need[2] = W.stiff = ballot(active && !(dk < 0x1.0p-3));
  W.next_resync = kResync;
  W.full_run = 0;
  W.calm = 0;
  W.vl_lo = K.vl_lo;
  W.vl_hi = K.vl_hi;
  asm volatile("" : "+s"(W.vl_lo), "+s"(W.vl_hi));  // opaque: values of their own, no longer parts of K's tuple (struct Wave)
}

__device__ __forceinline__ int wave_tier(const Wave &W) {
  return (W.need[2] & W.alive) ? FULL : ((W.need[1] & W.alive) ? WIDE : ((W.need[0] & W.alive) ? NARROW : TIGHT));
}

// the TIGHT trip with the in-step sum of squares (rk4_tight, INSTEP): step j squares the residual of its sample against obs[j];
// tsum = the trip's sum of them, from zero, so that the caller's running sum is not touched by a trip whose lane left the
// guard region (one add per trip, no copy kept for a restore).  Returns the wave's lanes that left it: the guard's compares
// as ballots, OR-ed as scalars — the same set as ballot(!guard_ok), without forming the per-lane flag.
// GUARD = false: the same steps with nothing measured (rk4_tight) — returns 0.
// The observations: the caller reads the first kObsAhead before the arithmetic (integrate_multi); the trip reads the others, a pair
// at every other step, kObsAhead steps before their own — far enough for the LDS latency, and the trip's top holds kObsAhead
// observations in registers in place of NU (twelve doubles fewer at NU = 16: the room the Series constants live in).
template <int NU>
constexpr int kObsAhead = NU < 4 ? NU : 4;
template <bool DAMP, int NU, bool GUARD = true>
__device__ __forceinline__ unsigned long long trip_fast_ssq(const double *v, const double (&head)[kObsAhead<NU>], const double *ob, const Lane &L,
                                                            const Series &S, const Consts &K, State &s, double &tsum) {
  static_assert(NU % 2 == 0, "the guard folds the figures of two steps (guard_note); observations come in pairs");
  constexpr int AH = kObsAhead<NU>;
  Guard g = {};
  double obs[NU];
#pragma unroll
  for (int j = 0; j < AH; ++j) obs[j] = head[j];
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    if (j % 2 == 0 && j + AH < NU) {
      obs[j + AH] = ob[j + AH];
      obs[j + AH + 1] = ob[j + AH + 1];
    }
    rk4_tight<DAMP, TIGHT, true, GUARD>(s, v[2 * j], v[2 * j + 1], v[2 * j + 2], L, K, g, obs[j], &tsum, j == 0, &S, (j & 1) != 0);
    // the guard's maxima are wanted only after the trip, and left alone the compiler gathers their instructions there, every
    // figure of the trip kept (and spilled: 700 bytes per lane) until then: made opaque, each pair of steps folds its own
    if constexpr (GUARD) {
      if (j & 1) asm volatile("" : "+v"(g.rho), "+v"(g.rho_f), "+v"(g.del), "+v"(g.del_e));
    }
  }
  if constexpr (!GUARD) return 0ull;
  return ballot(!(g.rho < S.lim_rho)) | ballot(!(g.rho_f < S.lim_c1)) | ballot(!(g.del < S.lim)) | ballot(!(g.del_e < S.lim_e));
}

// Can a lane's increments reach TIGHT's guard anywhere in the NU steps that start at s?  An A-PRIORI bound from the trip's start
// state (W0, Rh0) = (s.w, s.rx), the lane's constants and the range [vl_lo, vl_hi] of the loading table: where no lane of the wave
// needs the guard, the trip runs without it (trip_fast_ssq, GUARD = false) and is the guarded trip's to the bit.  Returns the
// lanes that DO need it.  Stated with the lane's limit on rho, Rl = min(2^-20, cbrt(2^-47 V_ref / |bh|)) (tight_rho_limit), Bl = Rl / 2,
// the constants R = 2^-20 >= Rl, B = 2^-21 >= Bl, Dmax = 0.9 * 2^-9 and, by induction over the trip's evaluations
// in order, the hypotheses that every stage derivative so far has |d1'| <= 0.9 Bl and every increment |dlt| <= D <= Dmax:
//   W    every step's end and every stage multiply the carried W by exp(dlt) to 4e-14 (the short series' truncation), so at any
//        stage of the trip W = W0 (1 + om) with |om| <= exp(NU D) - 1 + 1e-12 <= 1.02 NU D  (NU D <= NU Dmax < 0.035);
//   rho  a half-step stage's rho is a d1', the full-step stage's 2 c1, the step's end t1/3 with |t1| <= 6 max|d1'|: all <= 0.9 Rl
//        (<= 0.9 R, which is all the lines below use: where Rl is the smaller the hypotheses are tighter and nothing else changes);
//   Rh   moves by (1 + q) per step, |q| <= |rho| (1 + |rho|): over NU - 1 steps Rh = Rh0 (1 + rr), |rr| < NU 0.9 R (1 + 1e-5);
//   d0   = vl - vr W before the damping pass: |d0| <= max(|vl_hi - p|, |vl_lo - p|) + |p| gm1 =: D0,  p = vr W0, gm1 = 1.02 NU Dmax;
//        the pass, d0 -= W (d0 - brx d1') with |brx| = |bh (1 - rho)| <= |bh| (1 + R): |d0| <= D0 + Wm (D0 + |bh| B),  Wm = (1 + gm1) |W0|;
//   dlt  = dk - rho (b/a) (1 - rho/2) (the full-step stage: - 2 c1 (b/a)(1 - c1)) with |dk| <= |kh| max|d0| — the step's end takes
//        kh/6 times a sum of weight 6 —: |dlt| <= |kh| D0 + |b/a| R =: D.  Half-step stages: |khh| = |kh|/2 and |rho| <= 0.9 B: <= D/2;
//   d1'  = Rh - W xr, xr = xh (1 + dl) with dl in {0, a1, b1, 2 c1}, |dl| <= 0.9 R.  With c = Rh0 - W0 xh (the cancellation kept:
//        |Rh0| + |W0 xh| is thirty times too crude):  d1' = c + Rh0 rr - W0 xh (om + dl + om dl), and |W0 xh| <= |Rh0| + |c|, so
//        |d1'| <= |c| + (|Rh0| + |c|) (1.02 NU D + (NU + 1) R)    [0.9 (NU + 1.03 (1 + 1e-5)) <= NU + 1].
// D < Dmax and that last bound < 0.9 Bl (bmax: Series::bmax, the one per-lane figure) close the induction: |dlt| < 0.9 * 2^-9
// (half-step stages 0.9 * 2^-10), |c1| < 0.9 Bl, every |rho| < 0.9 Rl in exact arithmetic — the guard's own thresholds
// (trip_fast_ssq) with a tenth to spare; float64 rounding of the step and of these dozen operations is 1e-13 of that.
// Every quantity enters through its absolute value, so no sign of a constant is assumed, and a NaN anywhere makes a compare
// false: that lane needs the guard — today's path, whose guard lets NaN pass.
template <bool DAMP, int NU>
__device__ __forceinline__ unsigned long long tight_needs_guard(const State &s, const Lane &L, const Wave &W, float bmax) {
  using TB = TightBound<NU>;
  constexpr double R = TB::R, B = TB::B, Dmax = TB::Dmax, gm1 = TB::gm1;
  const double p = L.vrw * s.w;
  const double c = __builtin_fma(-s.w, L.hhdw, s.rx);  // (the first step's a1)
  double D0 = __builtin_fma(__builtin_fabs(p), gm1, __builtin_fmax(__builtin_fabs(W.vl_hi - p), __builtin_fabs(W.vl_lo - p)));
  if (DAMP) D0 = __builtin_fma((1.0 + gm1) * __builtin_fabs(s.w), __builtin_fma(__builtin_fabs(L.bh), B, D0), D0);
  const double D = __builtin_fma(__builtin_fabs(L.kh), D0, __builtin_fabs(L.boa) * R);
  const double rb = __builtin_fma(__builtin_fabs(s.rx) + __builtin_fabs(c), __builtin_fma(D, TB::G, TB::kap), __builtin_fabs(c));
  return ballot(!(D < Dmax)) | ballot(!(hi_as_float(rb) < bmax));
}

// samples completed by a trip of NU steps starting at chunk step r (dv[j]: the steps' V-derivative sums).  S1: every step
// is a sample, its observation obs[j] read ahead by the caller; else one every K.S steps (wave-uniform phase counter), V
// carried, the observation read from LDS where the sample completes (at most one per K.S >= 2 steps: selecting among
// observations read ahead by a run-time count costs a scratch array once that count is known to be scalar).
template <bool WANT_SSQ, bool WANT_ACC, bool S1, int NU>
__device__ __forceinline__ void emit_trip(const double (&dv)[NU], const double (&obs)[NU], const double *ld, int r, State &s, Emit &em,
                                          const Lane &L, const Consts &K, int k0, double &ssq, bool active, double *acc_out, int64_t stride) {
  if (S1) {
#pragma unroll
    for (int j = 0; j < NU; ++j) emit_incr<WANT_SSQ, WANT_ACC>(dv[j], r + j, obs[j], L, k0, ssq, active, acc_out, stride);
  } else {
#pragma unroll
    for (int j = 0; j < NU; ++j) {
      s.V = __builtin_fma(L.h6v, dv[j], s.V);
      if (++em.phase == K.S) {
        em.phase = 0;
        const double o = WANT_SSQ ? ld[em.ko] : 0.0;
        emit_sample<WANT_SSQ, WANT_ACC>(s.V, em, o, K, k0, ssq, active, acc_out, stride);
      }
    }
  }
}

// NU steps per trip through the loop (straight-line code): the resync test, the guard compare and the branch that waits
// for it, and the LDS addressing are paid per TRIP — and a lone wave sits out the whole latency of that
// compare-and-branch, ~150 cycles, whatever the trip holds (2 -> 4 -> 8 steps per trip: +12 %, +14 % at cfg1).
// Integrates trips of tier T from chunk step r while the wave's tier stays T; returns the first step not integrated.
// It comes back early — for integrate_tiers to re-decide the tier — when an alive lane's guard tripped (that trip is redone
// with full evaluations for the lane, which from then on needs the next wider tier), when no alive lane needs a tier this
// wide any more, or when no lane is alive.  All of that is ONE scalar branch at the end of the trip; the early-rejection
// compare uses the sum of squares as the PREVIOUS trip left it, so the branch never waits for the trip's last result.
constexpr int kTightUnroll = 8;  // steps per trip of the TIGHT loop (the one-parameter sampler runs 2 * kTightUnroll, rsf_kernels_sampler.h)
constexpr int kNarrowUnroll = 8, kWiderUnroll = 4;  // NARROW; WIDE
// INSTEP (TIGHT trips of a solve that wants the sum of squares alone, one step per sample: integrate_tiers): every step of
// the fast trip squares its own residual (trip_fast_ssq) — no dv[] exists on the hot path and each observation dies at
// its step.  The trip's sum joins ssq after the guard branch: the lanes in badmask drop it, restore the state and run the cold
// trip, whose samples join ssq one by one (trip_cold_ssq: observations read again); the others add the sum they hold.  The early-rejection compare
// reads ssq as the previous trip left it either way.
// UNGUARD (INSTEP, whole trips): the loop of the trips whose start state proves the guard idle (tight_needs_guard) — they run
// without it; at the first trip that does need it the loop sets W.guard_next and comes back without having taken that trip.
// The caller (integrate_tier) enters it only while no alive lane is in W.never.  The instance without UNGUARD is the guarded loop
// as it always was; for the whole trips of the in-step mode it comes back when the last lane of W.never has died, and after one
// trip when none held it in the first place (W.guard_next).  Two loops with one copy of the trip each: with both trips in one
// loop the guarded path lost 1.7 % at configs[1], with a third copy the kernels spilled to scratch memory.
template <bool DAMP, bool WANT_SSQ, bool WANT_ACC, int T, bool S1, int NU, bool INSTEP = false, bool UNGUARD = false>
__device__ __forceinline__ int integrate_multi(const double *lds, const double *ld, const Consts &K, Lane L, int k0, int kn, int r,
                                               int nsteps, State &s, Emit &em, double &ssq, double thr, bool active, double *acc_out,
                                               int64_t stride, Wave &W) {
  static_assert(NU >= 1 && (kResync % NU) == 0, "trip lengths divide the resync interval");
  static_assert(!INSTEP || (T == TIGHT && WANT_SSQ && !WANT_ACC && S1), "the in-step sum of squares: TIGHT, SSq alone, one step per sample");
  static_assert(!UNGUARD || (INSTEP && NU > 2), "whole trips of the in-step mode; the remainder's pairs keep the guard");
  constexpr bool HELD = INSTEP && NU > 2 && !UNGUARD;  // the guarded loop of whole in-step trips
  set_tier<T>(L);
  Series S;
  if constexpr (INSTEP) S = make_series<!UNGUARD>(L, K, s.rx);
  const bool held = HELD && (W.never & W.alive) != 0;  // (loop-invariant: W.never is read again only where a lane dies)
  for (; r + NU <= nsteps; r += NU) {
    const unsigned long long deadmask = WANT_SSQ ? ballot(ssq > thr) : 0ull;  // NaN compares false: such a lane runs on
    const double *v = lds + 2 * r;
    // one step per sample: the observations this trip completes, read before the arithmetic (a lone wave has nothing
    // else to hide the LDS latency behind)
    constexpr int NOBS = INSTEP ? kObsAhead<NU> : NU;  // (the in-step trip reads the others itself: trip_fast_ssq)
    double obs[NOBS], dv[INSTEP ? 1 : NU];
#pragma unroll
    for (int j = 0; j < NOBS; ++j) obs[j] = (WANT_SSQ && S1) ? ld[r + j] : 0.0;
    if constexpr (!INSTEP) {  // (the in-step trips carry (W, Rh) alone, with nothing to anchor them to: see kResync)
      if (r >= W.next_resync) {
        resync_t<DAMP, T>(s, L, K);
        W.next_resync = (r & ~(kResync - 1)) + kResync;
      }
    }
    if constexpr (UNGUARD) {
      // no alive lane can reach the guard from here: the trip without it — no saved state, nothing to compare afterwards, and
      // the branch back waits for nothing the trip computed.  The sum joins ssq as the guarded trip's does.
      if ((tight_needs_guard<DAMP, NU>(s, L, W, S.bmax) & W.alive) != 0) {
        W.guard_next = true;
        return r;
      }
      double usum = 0.0;
      trip_fast_ssq<DAMP, NU, false>(v, obs, ld + r, L, S, K, s, usum);
      W.ms_stale = true;
      W.steps[T] += NU;
      W.unguarded += NU;
      W.lane_steps += NU * (uint32_t)__builtin_popcountll(W.alive);
      ssq += usum;
      W.alive &= ~deadmask;
      if (W.alive == 0) return r + NU;
    } else {
    const State save = s;
    bool calm = false;
    double tsum = 0.0;
    unsigned long long tripped;
    if constexpr (INSTEP) tripped = trip_fast_ssq<DAMP, NU>(v, obs, ld + r, L, S, K, s, tsum);
    else tripped = ballot(trip_fast<DAMP, T, NU>(v, L, K, s, dv, &calm));
    const unsigned long long badmask = tripped & W.alive;  // wave-uniform, straight from the compares
    W.steps[T] += NU;
    W.lane_steps += NU * (uint32_t)__builtin_popcountll(W.alive);
    if constexpr (T != TIGHT) {  // evidence for one tier tighter: every alive lane calm in this trip (struct Wave)
      W.calm = (ballot(!calm) & W.alive) == 0 ? W.calm + NU : 0;
    }
    if (__builtin_expect(badmask != 0, 0)) {  // scalar branch: the hot path carries no exec-mask bookkeeping
      if (lane_in(badmask)) {
        s = save;
        if constexpr (INSTEP) {
          tsum = 0.0;  // the cold trip's samples instead, straight onto the running sum
          rebuild_ms<DAMP>(s, L);  // (the trips before this one left ms behind; the cold steps start from it)
          trip_cold_ssq<DAMP, T, NU>(v, ld + r, L, K, s, ssq);
        } else {
          trip_cold<DAMP, T, NU>(v, L, K, s, dv);
        }
      }
      W.need[T] |= badmask;
      W.redone += NU;
      W.full_run = 0;
      W.calm = 0;
    }
    if constexpr (INSTEP) {
      ssq += tsum;
      W.ms_stale = true;  // (a lane that went through the cold trip holds its ms; the others do not)
    } else emit_trip<WANT_SSQ, WANT_ACC, S1, NU>(dv, obs, ld, r, s, em, L, K, k0, ssq, active, acc_out, stride);
    const bool died = HELD && (deadmask & W.alive) != 0;
    W.alive &= ~deadmask;
    if constexpr (T != TIGHT) {
      if (W.calm >= kCalmSteps && badmask == 0) {  // demote: constant index (a run-time one would put the Wave in scratch memory)
        W.need[T - 1] &= ~W.alive | W.stiff;
        W.calm = 0;
      }
    }
    if (badmask != 0 || W.alive == 0 || (T != TIGHT && (W.need[T - 1] & W.alive) == 0)) return r + NU;
    if constexpr (HELD) {
      if (!held || (died && (W.never & W.alive) == 0)) return r + NU;
    }
    }
  }
  return r;
}

// The FULL tier: one step per trip with a full evaluation at every stage (rk4_cold), on the plain state (ms, x) — w and
// 1/x are not carried.  Runs while an alive lane needs it; every kFullRetry steps the lanes that came here from a tripped
// WIDE guard are sent back to try WIDE again.
template <bool DAMP, bool WANT_SSQ, bool WANT_ACC, bool S1>
__device__ __forceinline__ int integrate_full(const double *lds, const double *ld, const Consts &K, const Lane &L, int k0, int kn, int r,
                                              int nsteps, State &s, Emit &em, double &ssq, double thr, bool active, double *acc_out,
                                              int64_t stride, Wave &W) {
#pragma unroll 1
  for (; r < nsteps; ++r) {
    const unsigned long long deadmask = WANT_SSQ ? ballot(ssq > thr) : 0ull;
    const double *v = lds + 2 * r;
    const double obs[1] = {(WANT_SSQ && S1) ? ld[r] : 0.0};
    const double dv[1] = {rk4_cold<DAMP>(s, v[0], v[1], v[2], L, K)};
    W.steps[FULL] += 1;
    W.lane_steps += (uint32_t)__builtin_popcountll(W.alive);
    emit_trip<WANT_SSQ, WANT_ACC, S1, 1>(dv, obs, ld, r, s, em, L, K, k0, ssq, active, acc_out, stride);
    W.alive &= ~deadmask;
    if (++W.full_run >= kFullRetry) {
      W.need[2] &= W.stiff;
      W.full_run = 0;
    }
    if (W.alive == 0 || (W.need[2] & W.alive) == 0) return r + 1;
  }
  return r;
}

// Wave-uniform choice of the starting tier of the lockstep trajectories (integrate_lockstep below) — a speed decision
// only: every tier is exact to rounding inside its guard.  TIGHT and NARROW are tried whenever the mu increment allows it
// (|V_l - v| <~ 1.2 V_ref against their |dlt| guards 2^-9 / 2^-7): theta tracks its steady state closely (|dtheta/theta| ~ 1e-7
// per stage at Dc ~ 1000, h = 0.1), which no a-priori bound captures.  (The solve below decides the same per lane: wave_begin.)
__device__ __forceinline__ int start_tier(const Lane &L, const Consts &K) {
  const double dk = 1.2 * K.V_ref * K.h * L.kia;
  return !__any(!(dk < 0x1.0p-9)) ? TIGHT : (!__any(!(dk < 0x1.0p-7)) ? NARROW : WIDE);
}

// The lockstep driver, one staged chunk of kn output intervals: every lane of a wave takes the tier code through the chunk, trip
// by trip, in converged control flow, so that the caller's hooks may exchange values between lanes (init_kernel's groups,
// predict_kernel's ring).  The wave starts at start_tier and only ever moves to a wider tier, in trips of kLockstepTrip steps; a
// tripped guard sends that lane alone back to the trip's start and through it with full evaluations (trip_cold_plain); the
// chunk's last steps, fewer than a trip, go one at a time with the WIDE series.  (w, 1/x) are re-evaluated in full every
// kResync steps.  A chunk is a whole number of output intervals, so the interval's running sum starts and ends at zero here.
//   on_sample(ak, ko)  an output sample is complete: ak = cv * (the interval's V-derivative sums, like emit_incr), ko its index
//                      within the chunk's observations;
//   after_trip()       once after every trip.
// The caller keeps the chunk loop and stages the chunk, as solve() does (why: profiles/lockstep_driver).  solve() above is the
// sampler's per-lane tier machine (lanes leave early, tiers go both ways): different on purpose.
constexpr int kLockstepTrip = 8;
template <bool DAMP, typename OnSample, typename AfterTrip>
__device__ __forceinline__ void integrate_lockstep(double *lds, const Consts &K, const Lane &L, State &st, int kn, OnSample on_sample,
                                                   AfterTrip after_trip) {
  constexpr int NU = kLockstepTrip;
  static_assert(kResync % NU == 0, "the resync test looks at the first step of a trip");
  const int nsteps = K.S * kn;
  double dsum = 0.0;
  int phase = 0, ko = 0;  // RK4 steps since the last output sample; samples completed (both wave-uniform)
  // (every lane of the wave integrates — lanes past the last trajectory carry a harmless Dc = 1000 — so that the shuffles
  // and the wave-uniform tier decisions see whole waves)
  int tier = start_tier(L, K);
  int r = 0;
  auto trip = [&](auto tier_tag, auto nu_tag) {  // one trip of tier T, NUT steps; a tripped guard: that lane redoes it in full
    constexpr int T = decltype(tier_tag)::value, NUT = decltype(nu_tag)::value;
    const double *v = lds + 2 * r;
    Lane Lt = L;
    set_tier<T>(Lt);
    const State save = st;
    double dv[NUT];
    tier_enter<DAMP, T>(st, Lt);
    const bool bad = trip_fast<DAMP, T, NUT>(v, Lt, K, st, dv);
    tier_leave<DAMP, T>(st, Lt);
    const bool any_bad = ballot(bad) != 0;
    if (__builtin_expect(any_bad, 0)) {
      if (bad) {  // back to the trip's start (the plain state: saved before tier_enter) and through it with full evaluations
        st = save;
        trip_cold_plain<DAMP, NUT>(v, L, K, st, dv);
      }
    }
#pragma unroll
    for (int j = 0; j < NUT; ++j) {
      dsum += dv[j];
      if (++phase == K.S) {
        phase = 0;
        on_sample(dsum * L.cv, ko);
        dsum = 0.0;
        ++ko;
      }
    }
    return any_bad;
  };
  for (; r + NU <= nsteps; r += NU) {
    if ((r & (kResync - 1)) == 0) eval_full(st.ms, st.x, L, K, st.w, st.rx);
    bool any_bad;
    if (tier == TIGHT) any_bad = trip(std::integral_constant<int, TIGHT>{}, std::integral_constant<int, NU>{});
    else if (tier == NARROW) any_bad = trip(std::integral_constant<int, NARROW>{}, std::integral_constant<int, NU>{});
    else any_bad = trip(std::integral_constant<int, WIDE>{}, std::integral_constant<int, NU>{});
    if (any_bad && tier < WIDE) ++tier;
    after_trip();
  }
  for (; r < nsteps; ++r) {  // fewer than NU steps left in the chunk: one at a time
    if ((r & (kResync - 1)) == 0) eval_full(st.ms, st.x, L, K, st.w, st.rx);
    trip(std::integral_constant<int, WIDE>{}, std::integral_constant<int, 1>{});
    after_trip();
  }
}

// trips of tier T from chunk step r (at least two steps are left): long trips while they fit, then pairs
template <bool DAMP, bool WANT_SSQ, bool WANT_ACC, int T, bool S1, int NU, bool INSTEP = false>
__device__ __forceinline__ int integrate_tier(const double *lds, const double *ld, const Consts &K, const Lane &L, int k0, int kn, int r,
                                              int nsteps, State &s, Emit &em, double &ssq, double thr, bool active, double *acc_out,
                                              int64_t stride, Wave &W) {
  if (r + NU <= nsteps) {
    if constexpr (INSTEP) {  // the trips that may drop the guard, unless a lane of W.never holds the wave to the guarded loop
      if ((W.never & W.alive) == 0 && !W.guard_next) return integrate_multi<DAMP, WANT_SSQ, WANT_ACC, T, S1, NU, true, true>(lds, ld, K, L, k0, kn, r, nsteps, s, em, ssq, thr, active, acc_out, stride, W);
    }
    W.guard_next = false;
    return integrate_multi<DAMP, WANT_SSQ, WANT_ACC, T, S1, NU, INSTEP>(lds, ld, K, L, k0, kn, r, nsteps, s, em, ssq, thr, active, acc_out, stride, W);
  }
  return integrate_multi<DAMP, WANT_SSQ, WANT_ACC, T, S1, 2, INSTEP>(lds, ld, K, L, k0, kn, r, nsteps, s, em, ssq, thr, active, acc_out, stride, W);
}

// SSQ_IN_STEP: the caller wants the TIGHT trips' in-step sum of squares (integrate_multi, INSTEP) where the solve allows it —
// the sum of squares alone, one step per sample.  The sampler asks for it; the forward kernel's SSq-only launch does not: it
// returns the trajectory launch's sum to the bit.
template <bool DAMP, bool WANT_SSQ, bool WANT_ACC, bool S1, int NUT, bool SSQ_IN_STEP>
__device__ __forceinline__ void integrate_tiers(const double *lds, const double *ld, const Consts &K, const Lane &L, int k0,
                                                int kn, State &s, double &ssq, double thr, bool active, double *acc_out, int64_t stride, Wave &W) {
  constexpr bool INSTEP = SSQ_IN_STEP && WANT_SSQ && !WANT_ACC && S1;
  const int nsteps = S1 ? kn : K.S * kn;
  Emit em = {0, 0, s.V};
  int r = 0;
  W.next_resync = kResync;  // chunk-local; not at a chunk's first step (see kResync)
  bool scaled = false;      // s.rx holds Rh = hhd / x and s.w holds W (the incremental tiers' state) rather than 1 / x and w
  while (r < nsteps && W.alive != 0) {
    const int tier = wave_tier(W);
    if constexpr (INSTEP) {
      // in-step trips have run and something else comes next (another tier, the chunk's odd last step): ms from (W, Rh) before
      // a cold step, a resync or the FULL tier reads it, and the resync interval counted from here, where ms and (W, Rh) agree.
      // Out of line of the in-step loops: their register allocation does not see it.
      if (W.ms_stale && (tier != TIGHT || nsteps - r == 1)) {
        rebuild_ms<DAMP>(s, L);  // (scaled: only the incremental tiers set the flag)
        W.ms_stale = false;
        W.next_resync = (r & ~(kResync - 1)) + kResync;
      }
    }
    if (tier == FULL) {
      if (scaled) { tier_leave<DAMP, WIDE>(s, L); scaled = false; }
      r = integrate_full<DAMP, WANT_SSQ, WANT_ACC, S1>(lds, ld, K, L, k0, kn, r, nsteps, s, em, ssq, thr, active, acc_out, stride, W);
      eval_full(s.ms, s.x, L, K, s.w, s.rx);  // (w, 1/x) at the point the incremental tiers — or the next chunk — continue from
      continue;
    }
    if (!scaled) { tier_enter<DAMP, TIGHT>(s, L); scaled = true; }
    // the chunk's odd last step (it always completes a sample): with the WIDE series whatever the tier — one instance
    if (nsteps - r == 1) r = integrate_multi<DAMP, WANT_SSQ, WANT_ACC, WIDE, S1, 1>(lds, ld, K, L, k0, kn, r, nsteps, s, em, ssq, thr, active, acc_out, stride, W);
    else if (tier == TIGHT) r = integrate_tier<DAMP, WANT_SSQ, WANT_ACC, TIGHT, S1, NUT, INSTEP>(lds, ld, K, L, k0, kn, r, nsteps, s, em, ssq, thr, active, acc_out, stride, W);
    else if (tier == NARROW) r = integrate_tier<DAMP, WANT_SSQ, WANT_ACC, NARROW, S1, kNarrowUnroll>(lds, ld, K, L, k0, kn, r, nsteps, s, em, ssq, thr, active, acc_out, stride, W);
    else r = integrate_tier<DAMP, WANT_SSQ, WANT_ACC, WIDE, S1, kWiderUnroll>(lds, ld, K, L, k0, kn, r, nsteps, s, em, ssq, thr, active, acc_out, stride, W);
  }
  if constexpr (INSTEP) {
    if (scaled && W.ms_stale && k0 + kn < K.nout) {  // the next chunk may start with anything; after the last one nobody reads ms
      rebuild_ms<DAMP>(s, L);
      W.ms_stale = false;
    }
  }
  if (scaled) tier_leave<DAMP, WIDE>(s, L);
}

// Integrate kn output intervals from the staged chunk.  Accumulates the sum of squares
// (MCMC.py:387) and optionally stores acc time-major (`active` lanes only).  Called by whole waves.
template <bool DAMP, bool WANT_SSQ, bool WANT_ACC, int NUT, bool SSQ_IN_STEP>
__device__ __forceinline__ void integrate_chunk(const double *lds, const Consts &K, const Lane &L, int k0, int kn, State &s,
                                                double &ssq, double thr, bool active, double *acc_out, int64_t stride, Wave &W) {
  const double *ld = lds + lds_data_offset(K);
  if (K.S == 1) integrate_tiers<DAMP, WANT_SSQ, WANT_ACC, true, NUT, SSQ_IN_STEP>(lds, ld, K, L, k0, kn, s, ssq, thr, active, acc_out, stride, W);
  else integrate_tiers<DAMP, WANT_SSQ, WANT_ACC, false, NUT, SSQ_IN_STEP>(lds, ld, K, L, k0, kn, s, ssq, thr, active, acc_out, stride, W);
}

// Full forward solve for one lane.  Every thread of the workgroup must call it (chunk staging has barriers);
// `resident` (workgroup-uniform): the single chunk is already staged, nothing is re-staged.
// NUT: RK4 steps per trip of the TIGHT loop (integrate_multi); 16 where the kernel's registers allow it (one-parameter
// sampler), 8 otherwise.  thr: a sum of squares above it cannot be accepted (struct Wave; +inf where every lane's result is
// wanted) — the value returned for a lane that stopped counting is the partial sum that disqualified it.  W: the solve's
// wave-level control and statistics, for the caller's counters.  SSQ_IN_STEP: integrate_tiers.
template <bool DAMP, bool WANT_SSQ, bool WANT_ACC, int NUT = kTightUnroll, bool SSQ_IN_STEP = false>
__device__ __forceinline__ double solve(double *lds, const Consts &K, bool resident, bool active, double dc, double a,
                                        double b, double thr, double *acc_out, int64_t stride, Wave &W) {
  const Lane L = make_lane<DAMP>(dc, a, b, K);
  State s = initial_state(dc, L, K);
  wave_begin<NUT>(W, active, L, K);
  double ssq = 0.0;
  if (WANT_ACC && active) acc_out[0] = 0.0;
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    if (!resident) stage_chunk(lds, K, k0, kn);
    if (WANT_SSQ && k0 == 1) {  // sample 0 belongs to no chunk: acc[0] = 0, RateStateModel.py:371 (staged with every chunk)
      const double d0 = lds[lds_d0_offset(K)];
      ssq = d0 * d0;
    }
    // a wave-uniform branch: every lane of a wave with work goes in — the lanes that are not `active` (out of bounds, past
    // the end of the batch) ride along masked out of W.alive and of the trajectory stores.  (Under `if (active)`, a divergent
    // branch, everything the solve leaves in W would count as divergent after it and move from scalar to vector registers.)
    if (W.alive != 0) integrate_chunk<DAMP, WANT_SSQ, WANT_ACC, NUT, SSQ_IN_STEP>(lds, K, L, k0, kn, s, ssq, thr, active, acc_out, stride, W);
  }
  return ssq;
}

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. SC'11; Random123 constants) and the variates built on it.
// counter = (chain_lo, chain_hi, iteration, slot), key = seed.  Slots of one (chain, iteration):
//   0: proposal normals z0,z1   1: z2   2: accept uniform   8+2j / 9+2j: gamma attempt j
// ---------------------------------------------------------------------------------------------
enum : uint32_t { SLOT_Z01 = 0, SLOT_Z2 = 1, SLOT_U = 2, SLOT_GAMMA = 8 };

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ void draw_words(uint64_t seed, uint64_t chain, uint32_t iter, uint32_t slot,
                                           uint32_t w[4]) {
  philox4x32_10((uint32_t)chain, (uint32_t)(chain >> 32), iter, slot, (uint32_t)seed, (uint32_t)(seed >> 32), w);
}

// 53-bit uniform in (0, 1]
__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {
  const uint64_t k = (((uint64_t)hi << 32) | lo) >> 11;
  return (double)(k + 1) * 0x1.0p-53;
}

// The variates use the kernel's own log / sincos (rsf_math.h, <= 4 ulp): the oracle's libm values differ in the last
// bits, which matters only when an accept test sits within ~1e-15 of its threshold (tests: draws to 1e-12).
__device__ __forceinline__ void normal_pair(const uint32_t w[4], double &z0, double &z1) {
  const double u1 = u53(w[0], w[1]), u2 = u53(w[2], w[3]);
  const double r = sqrt(-2.0 * fm::log(u1));
  double s, c;
  fm::sincos2pi(u2, s, c);
  z0 = r * c;
  z1 = r * s;
}

__device__ __forceinline__ double rng_log(double x) { return fm::log(x); }

// Marsaglia & Tsang (2000), shape >= 1, log acceptance test only.  d = shape - 1/3 and c = 1/sqrt(9 d) come from
// the host (chain-independent).
__device__ __forceinline__ double gamma_draw(uint64_t seed, uint64_t chain, uint32_t iter, double d, double c) {
  for (uint32_t j = 0; j < 64; ++j) {
    uint32_t w[4];
    double x, unused;
    draw_words(seed, chain, iter, SLOT_GAMMA + 2 * j, w);
    normal_pair(w, x, unused);
    double v = 1.0 + c * x;
    if (!(v > 0.0)) continue;
    v = v * v * v;
    draw_words(seed, chain, iter, SLOT_GAMMA + 2 * j + 1, w);
    const double u = u53(w[0], w[1]);
    if (rng_log(u) < 0.5 * x * x + d * (1.0 - v + rng_log(v))) return d * v;
  }
  return d;
}

// ---------------------------------------------------------------------------------------------
// small dense helpers, fully unrolled on the compile-time dimension
// ---------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ bool chol_lower(const double *V, double *L) {
  bool ok = true;
#pragma unroll
  for (int e = 0; e < D * D; ++e) L[e] = 0.0;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double s = V[j * D + j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j * D + k] * L[j * D + k];
    if (!(s > 0.0)) { ok = false; continue; }
    const double ljj = sqrt(s);
    L[j * D + j] = ljj;
#pragma unroll
    for (int i = j + 1; i < D; ++i) {
      double t = V[i * D + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i * D + k] * L[j * D + k];
      L[i * D + j] = t / ljj;
    }
  }
  return ok;
}

template <int D>
__device__ __forceinline__ void sym_inverse(const double *A, double *Ai) {
  if (D == 1) {
    Ai[0] = 1.0 / A[0];
  } else {
    const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const double id = 1.0 / (A[0] * c00 + A[1] * c01 + A[2] * c02);
    Ai[0] = c00 * id; Ai[1] = (A[2] * A[7] - A[1] * A[8]) * id; Ai[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    Ai[3] = c01 * id; Ai[4] = (A[0] * A[8] - A[2] * A[6]) * id; Ai[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    Ai[6] = c02 * id; Ai[7] = (A[1] * A[6] - A[0] * A[7]) * id; Ai[8] = (A[0] * A[4] - A[1] * A[3]) * id;
  }
}

// scale * (cov + diag(eps)) from shifted sums ws[p] = sum (q_p - ref_p), wq[p][r] = sum (q_p - ref_p)(q_r - ref_r) over nn
// samples (ddof = 1, like np.cov), and its lower Cholesky factor.  false: not positive definite (the caller keeps its
// covariance; with eps > 0 that does not happen).  This is the corrected adaptive Metropolis of `adapt_mode = am`
// (Haario, Saksman & Tamminen 2001): the sums run over the chain's WHOLE history since rsf_mcmc_init — adaptation that
// diminishes, so the chain still converges to the posterior — and eps_p = (1e-6 (hi_p - lo_p))^2 keeps the matrix positive
// definite when the history holds fewer than D + 1 distinct points.  (Until round 4 `am` used the last adapt_interval samples
// only, as the reference's broken update does: measured on the three-parameter problem, that shifts the pooled posterior —
// the mean of Dc*a by 89 standard errors, its spread by 8 % — because a proposal that forgets is a different chain, not an
// adaptive one; and a window with too few distinct points made "positive definite" a coin toss of the last bit.)
template <int D>
__device__ __forceinline__ bool window_covariance(const double *ws, const double *wq, double nn, double scale, const double *eps, double *Vn,
                                                  double *Ln) {
#pragma unroll
  for (int p = 0; p < D; ++p)
#pragma unroll
    for (int r = 0; r < D; ++r) Vn[p * D + r] = scale * ((wq[p * D + r] - ws[p] * ws[r] / nn) / (nn - 1.0) + (p == r ? eps[p] : 0.0));
  return chol_lower<D>(Vn, Ln);
}

// np.cov of ONE variable's window as NumPy forms it (numpy/lib/_function_base_impl.py::cov): the mean from np.add.reduce's
// pairwise summation — fewer than 8 elements one by one from 0; up to 128 (RSF_DICT_MAX_INTERVAL) through eight interleaved
// accumulators combined pairwise, the remainder one by one (numpy/_core/src/umath/loops_utils.h.src) — then the
// deviations' dot product times 1 / (n - 1).  The ORDER of that sum is what `reference_dict` adaptation needs: whether the
// mean of a window of identical samples is that sample (covariance exactly 0: np.linalg.cholesky raises and the reference
// keeps its proposal, MCMC.py:524-527) or one ulp off (covariance ~1e-31: the Cholesky "succeeds" and the reference's
// proposal collapses to ~1e-8) depends on the sample's low bits through exactly these additions.  a(k): sample k.
template <typename F>
__device__ __forceinline__ double np_cov_1d(F a, int n) {
  double sum;
  if (n < 8) {
    sum = 0.0;
    for (int i = 0; i < n; ++i) sum += a(i);
  } else {
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a(j);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] += a(i + j);
    sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) sum += a(i);
  }
  const double avg = sum / (double)n;
  double c = 0.0;
  for (int k = 0; k < n; ++k) {
    const double dlt = a(k) - avg;
    c = __builtin_fma(dlt, dlt, c);
  }
  return c * (1.0 / (double)(n - 1));
}

}  // namespace rsf
