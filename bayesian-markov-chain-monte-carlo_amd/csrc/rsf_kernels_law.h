// rsf_kernels_law.h — the state-law family (include/rsf_law.h): law_forward_kernel, the plain float64 RK4 solve under the ageing
// or the slip law.  Included by rsf_law.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsf_law.h"
#include "rsf_kernel_common.h"
#include "rsf_device.h"

namespace rsfk {

// One full evaluation of the RHS at (ms, x) under LAW: rsf::eval_full and rsf::rhs_tail with the d(theta)/dt line switched.
// eval_full's exponent e = ms k'/a - mu_ref/a - (b/a) lx (w = exp e) and lx = log x are formed anyway, and log(v theta / Dc) =
// log(w x) = e + lx: the slip law costs one add and one product more than the ageing law.  d0, d1, d2: rhs_tail's.
template <int LAW, bool DAMP>
__device__ __forceinline__ void law_rhs(double ms, double x, double vl, const rsf::Lane &L, const Consts &K, double &d0, double &d1, double &d2) {
  const double lx = rsf::fm::log(x);
  const double e = __builtin_fma(-L.boa, lx, __builtin_fma(ms, L.kia, L.tc));
  const double w = rsf::fm::exp(e), rx = rsf::fm::rcp(x);
  if (LAW == RSF_LAW_SLIP) d1 = -(w * x) * (e + lx);   // slip law: -(v theta / Dc) log(v theta / Dc)
  else d1 = __builtin_fma(-w, x, 1.0);                 // ageing law: 1 - v theta / Dc
  d0 = __builtin_fma(-K.V_ref, w, vl);                 // V_l - v
  const double bt = (L.beta * d1) * rx;                // b / theta d(theta)/dt, in units of k'
  double g = d0 - bt;
  if (DAMP) {                                          // the single damping pass, RateStateModel.py:349-353
    const double kw = L.kvk * w;
    d0 = __builtin_fma(-kw, g, d0);
    g = d0 - bt;
    d2 = kw * g;
  } else {
    d2 = w * g;
  }
}

// rsf::rk4_cold's arithmetic on the plain state (ms, x): the step's weighted V-derivative sum in Lane::h6v's units
template <int LAW, bool DAMP>
__device__ __forceinline__ double law_step(double &ms, double &x, double vl0, double vlm, double vl1, const rsf::Lane &L, const Consts &K) {
  double k0 = 0.0, k1 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma nounroll
  for (int st = 0; st < 4; ++st) {
    const double c = st == 0 ? 0.0 : (st == 3 ? K.h : K.hh);
    const double wgt = (st == 0 || st == 3) ? 1.0 : 2.0;
    const double vl = st == 0 ? vl0 : (st == 3 ? vl1 : vlm);
    double d0, d1, d2;
    law_rhs<LAW, DAMP>(__builtin_fma(c, k0, ms), __builtin_fma(c * L.vdc, k1, x), vl, L, K, d0, d1, d2);
    s0 = __builtin_fma(wgt, d0, s0);
    s1 = __builtin_fma(wgt, d1, s1);
    s2 = __builtin_fma(wgt, d2, s2);
    k0 = d0;
    k1 = d1;
  }
  ms = __builtin_fma(K.h6, s0, ms);
  x = __builtin_fma(L.h6d, s1, x);
  return s2;
}

// One lane per parameter set (dc, a, b); a, b NULL: the model's.  The loading table and the observation go through LDS chunk by
// chunk (rsf::stage_chunk: every thread of the workgroup stages, whatever its lane's state).  ssq_out / acc_out NULL: not
// wanted (K.data is NULL without ssq_out); acc_out is time-major [nout][n].  A wave whose lanes are all past n stages and
// skips the steps; a lane past n in a wave with work rides along with a harmless point and stores nothing.  No atomics, no
// scratch, no tier: a NaN trajectory runs to the end.
template <int LAW, bool DAMP>
__global__ void __launch_bounds__(kMaxBlock)
law_forward_kernel(Consts K, int64_t n, const double *__restrict__ dc, const double *__restrict__ a, const double *__restrict__ b,
                   double *__restrict__ ssq_out, double *__restrict__ acc_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  const bool want_ssq = ssq_out != nullptr, want_acc = acc_out != nullptr;
  const double dci = active ? dc[i] : 1000.0;
  const rsf::Lane L = rsf::make_lane<DAMP>(dci, (active && a) ? a[i] : K.a_def, (active && b) ? b[i] : K.b_def, K);
  const rsf::State s0 = rsf::initial_state(dci, L, K);
  double ms = s0.ms, x = s0.x, V = s0.V, vprev = s0.V, ssq = 0.0;
  double *acc_i = want_acc ? acc_out + i : nullptr;
  if (want_acc && active) acc_i[0] = 0.0;                // acc_0 = 0, RateStateModel.py:371
  const bool work = rsf::ballot(active) != 0;            // wave-uniform
  const double *ld = lds + rsf::lds_data_offset(K);
  int phase = 0;                                         // RK4 steps since the last output sample (wave-uniform)
  for (int k0 = 1; k0 < K.nout; k0 += K.kc) {
    const int kn = min(K.kc, K.nout - k0);
    rsf::stage_chunk(lds, K, k0, kn);
    if (want_ssq && k0 == 1) {
      const double d0 = lds[rsf::lds_d0_offset(K)];
      ssq = d0 * d0;                                     // (acc_0 - data_0)^2
    }
    if (!work) continue;
    const int nsteps = K.S * kn;
    int ko = 0;
    for (int r = 0; r < nsteps; ++r) {
      const double *v = lds + 2 * r;
      V = __builtin_fma(L.h6v, law_step<LAW, DAMP>(ms, x, v[0], v[1], v[2], L, K), V);
      if (++phase == K.S) {
        phase = 0;
        if (want_acc) rsf::emit_at<false, true>(V, vprev, ko, 0.0, K, k0, ssq, active, acc_i, n);
        if (want_ssq) rsf::emit_at<true, false>(V, vprev, ko, ld[ko], K, k0, ssq, active, nullptr, 0);
        vprev = V;
        ++ko;
      }
    }
  }
  if (want_ssq && active) ssq_out[i] = ssq;
}

}  // namespace rsfk
