// rsf_kernels_observe.h — the observables of the state-law solve (include/rsf_observe.h): law_observe_kernel, law_forward_kernel's
// plain float64 RK4 under either law with the output sample chosen by the caller: the acceleration, the friction coefficient, the
// state variable or the slip velocity.  Included by rsf_observe.hip and, for the sample rule, by rsf_kernels_law_dr.h.  The
// arithmetic of the solve is rsf_kernels_law.h's law_rhs / law_step, called from here, not restated.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_observe.h"
#include "rsf_kernels_law.h"

namespace rsfk {

// The residual of an output sample that is a value of the trajectory itself (every observable but the acceleration): s is the
// ROUNDED value that is stored — contraction is off here, so that r is not formed as fma(factor, state, -obs) from an unrounded
// product and the sum of squares is the stored series' own.
__device__ __forceinline__ double observe_residual(double s, double obs) {
#pragma clang fp contract(off)
  return s - obs;
}

// The sample rule of an observable, defined ONCE for law_observe_kernel and the fused sampler's solve (rsf_kernels_law_dr.h):
// sample k >= 1 from the state after the sample's last step, and its residual against obs; vprev: the V of the sample before
__device__ __forceinline__ void observe_sample(int32_t observable, double V, double &vprev, double ms, double x, double scale, double obs,
                                               const Consts &K, double &s, double &res) {
  switch (observable) {
    case RSF_OBS_ACC: {
      // rsf::emit_at's sample and residual AS law_forward_kernel COMPILES THEM: the stored sample is the rounded product,
      // the residual ak - obs one fma of the velocity difference (the compiler contracts emit_at's product into it).  Written
      // out, because beside the other cases the compiler shares the rounded product instead, an ulp of SSq away.
      const double dv = V - vprev;
      s = dv * K.inv_dt;
      res = __builtin_fma(dv, K.inv_dt, -obs);
      vprev = V;
    } break;
    case RSF_OBS_VELOCITY: s = V; res = observe_residual(s, obs); break;
    case RSF_OBS_MU: s = scale * ms; res = observe_residual(s, obs); break;
    default: s = x * scale; res = observe_residual(s, obs); break;  // RSF_OBS_THETA (the host admits no other)
  }
}

// law_forward_kernel's solve — one lane per (dc, a, b), the loading table and the observation through LDS chunk by chunk, a wave
// past n staging and skipping the steps, a lane past n riding along with a harmless point — with `observable` (RSF_OBS_*, a kernel
// argument: wave-uniform, so its branch is scalar and taken once per output sample, K.S steps, outside law_step) choosing
// sample k >= 1 from the state after the sample's last step:
//   RSF_OBS_ACC       (V_k - V_{k-1}) inv_dt, rsf::emit_at's: this kernel then returns law_forward_kernel's results bit for bit
//   RSF_OBS_VELOCITY  the carried V
//   RSF_OBS_MU        L.kprime * ms: mu = k' ms, ONE product of the rounded k' = 0.1 (1 / Dc) of make_lane and the state
//   RSF_OBS_THETA     x * (dc * K.inv_vref): theta = x Dc / V_ref as the state times the ROUNDED product Dc (1 / V_ref), 1 / V_ref
//                     the host's rounded reciprocal — three roundings from the exact x Dc / V_ref, none of them a division
// and sample 0 the initial value: 0, V_ref, kprime * ms_0, x_0 * (dc * inv_vref).  The sum of squares is the running
// fma(r, r, ssq) of r = s_k - data_k from k = 0, its first term (s_0 - data_0)^2: data_0^2 for the acceleration, as
// law_forward_kernel's.  ssq_out / series_out NULL: not wanted (K.data is NULL without ssq_out); series_out is time-major
// [nout][n].  No atomics, no scratch, no tier, no guard: a NaN trajectory runs to the end.
template <int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock)
law_observe_kernel(Consts K, int32_t observable, int64_t n, const double *__restrict__ dc, const double *__restrict__ a,
                   const double *__restrict__ b, double *__restrict__ ssq_out, double *__restrict__ series_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  const bool want_ssq = ssq_out != nullptr, want_series = series_out != nullptr;
  const double dci = active ? dc[i] : 1000.0;
  const rsf::Lane L = rsf::make_lane<DAMP>(dci, (active && a) ? a[i] : K.a_def, (active && b) ? b[i] : K.b_def, K);
  const rsf::State s0 = rsf::initial_state(dci, L, K);
  double ms = s0.ms, x = s0.x, V = s0.V, vprev = s0.V, ssq = 0.0;
  // the one per-lane factor a sample takes: Dc / V_ref for the state variable, k' otherwise (read by the friction alone)
  const double scale = observable == RSF_OBS_THETA ? dci * K.inv_vref : L.kprime;
  const double first = observable == RSF_OBS_ACC ? 0.0                     // acc_0 = 0, RateStateModel.py:371
                       : observable == RSF_OBS_VELOCITY ? s0.V
                       : observable == RSF_OBS_MU ? scale * s0.ms : s0.x * scale;
  double *series_i = want_series ? series_out + i : nullptr;
  const bool store = want_series && active;
  if (store) series_i[0] = first;
  const bool work = rsf::ballot(active) != 0;            // wave-uniform
  const double *ld = lds + rsf::lds_data_offset(K);
  int phase = 0;                                         // RK4 steps since the last output sample (wave-uniform)
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    rsf::stage_chunk(lds, K, k0, kn);
    if (want_ssq && k0 == 1) {
      const double r0 = first - lds[rsf::lds_d0_offset(K)];
      ssq = r0 * r0;                                     // (s_0 - data_0)^2
    }
    if (!work) continue;
    const int nsteps = K.S * kn;
    int ko = 0;
    for (int r = 0; r < nsteps; ++r) {
      const double *v = lds + 2 * r;
      V = __builtin_fma(L.h6v, law_step<LAW, DAMP>(ms, x, v[0], v[1], v[2], L, K), V);
      if (++phase == K.S) {
        phase = 0;
        const double obs = want_ssq ? ld[ko] : 0.0;
        double s, res;                                   // the sample and its residual
        observe_sample(observable, V, vprev, ms, x, scale, obs, K, s, res);
        if (store) series_i[(int64_t)(k0 + ko) * n] = s;
        if (want_ssq) ssq = __builtin_fma(res, res, ssq);
        ++ko;
      }
    }
  }
  if (want_ssq && active) ssq_out[i] = ssq;
}

}  // namespace rsfk
