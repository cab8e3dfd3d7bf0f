// rsf_kstiff.hip — the delayed-rejection sampler of the state-law solve with the spring's stiffness among the parameters
// (include/rsf_kstiff.h): rsf_kstiff_observe / _dr_run / _dr_ssq / _dr_propose / _dr_accept (kernels: rsf_kernels_kstiff.h; the
// argument checks are rsf_dr.hip's, rsf_law_dr.hip's and rsf_stiff.hip's: rsf_dr_host.h).
#include <cmath>
#include <vector>

#include "rsf_dr_host.h"
#include "rsf_kernels_kstiff.h"

using namespace rsfk;
using namespace rsfh;

// KDrArgs' chains are (Dc, k) or (Dc, a, b, k): set_chains asks for d = 2 or 4
template <> struct rsfh::stiffness_last<KDrArgs> : std::true_type {};

namespace {

auto observe_fn(const rsf_ctx *c, int law) {
  return with<RSF_LAW_SLIP, RSF_LAW_AGEING>(law, [&](auto LAW) {
    return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return kstiff_observe_kernel<LAW, DAMP>; });
  });
}
template <class F> auto kstiff_dr_fn(const rsf_ctx *c, int d, int law, F pick) {
  return with<2, 4>(d, [&](auto D) {
    return with<RSF_LAW_SLIP, RSF_LAW_AGEING>(law, [&](auto LAW) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return pick(D, LAW, DAMP); }); });
  });
}
auto run_fn(const rsf_ctx *c, int d, int law) {
  return kstiff_dr_fn(c, d, law, [](auto D, auto LAW, auto DAMP) { return kstiff_dr_kernel<D, LAW, DAMP>; });
}
auto ssq_fn(const rsf_ctx *c, int d, int law) {
  return kstiff_dr_fn(c, d, law, [](auto D, auto LAW, auto DAMP) { return kstiff_dr_ssq_kernel<D, LAW, DAMP>; });
}
auto propose_fn(int d) { return with<2, 4>(d, [](auto D) { return kstiff_dr_propose_kernel<D>; }); }
auto accept_fn(int d) { return with<2, 4>(d, [](auto D) { return kstiff_dr_accept_kernel<D>; }); }

// the model's integrator: what the calls that solve refuse beyond rsf_dr.hip's checks
int check_integrator(const char *fn, const rsf_ctx *c) {
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "%s: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)", fn);
  return RSF_OK;
}

// the box of the stiffness, the last of d coordinates, lies in k > 0 (after set_chains: d is 2 or 4 and the box is finite)
int check_stiffness_box(const char *fn, int32_t d, const double *lo) {
  if (!(lo[d - 1] > 0.0)) return fail(RSF_ERR_INVALID, "%s: need lo[%d] > 0: the box of the stiffness, the last coordinate, lies in k > 0", fn, d - 1);
  return RSF_OK;
}

}  // namespace

extern "C" {

int rsf_kstiff_observe(rsf_ctx *c, int32_t law, int32_t observable, int64_t n, const double *dc, const double *a, const double *b, const double *k,
                       const double *data, double *ssq_out, double *series_out) {
  RSF_ENTER(c, NEED_MODEL, dc && k && n >= 0, "bad argument");
  int rc;
  if ((rc = check_law(__func__, law, observable))) return rc;
  if (ssq_out && !data) return fail(RSF_ERR_INVALID, "rsf_kstiff_observe: ssq_out needs data");
  if ((rc = check_integrator(__func__, c))) return rc;
  if (n == 0) return RSF_OK;
  const size_t nb = (size_t)n * sizeof(double);
  // every k[i] finite and > 0, read on the host: a device caller's array from a copy
  std::vector<double> copy;
  const double *hk = k;
  if (!host_mem(c)) {
    copy.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(copy.data(), k, nb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    hk = copy.data();
  }
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(hk[i]) || !(hk[i] > 0.0)) return fail(RSF_ERR_INVALID, "rsf_kstiff_observe: k[%lld] must be finite and > 0", (long long)i);
  if (!ssq_out && !series_out) return RSF_OK;
  const double *ddc, *da, *db, *dk, *ddata;
  double *dssq, *dser;
  if ((rc = stage_in(c, SLOT_DC, dc, nb, &ddc))) return rc;
  if ((rc = stage_in(c, SLOT_A, a, nb, &da))) return rc;
  if ((rc = stage_in(c, SLOT_B, b, nb, &db))) return rc;
  if ((rc = stage_in(c, SLOT_STIFFNESS, k, nb, &dk))) return rc;
  if ((rc = stage_in(c, SLOT_DATA, ssq_out ? data : nullptr, (size_t)c->nout * sizeof(double), &ddata))) return rc;
  if ((rc = stage_out(c, SLOT_SSQ_OUT, ssq_out, nb, &dssq))) return rc;
  if ((rc = stage_out(c, SLOT_ACC_OUT, series_out, nb * (size_t)c->nout, &dser))) return rc;
  // the shared chunking of the float64 tables (c->kc, c->lds_bytes), as rsf_stiff_observe
  if ((rc = launch(c, observe_fn(c, law), grid_for(c, n), c->block, c->lds_bytes, make_consts(c, ddata), observable, n, ddc, da, db, dk, dssq, dser)))
    return rc;
  if ((rc = copy_back(c, SLOT_SSQ_OUT, ssq_out, nb))) return rc;
  if ((rc = copy_back(c, SLOT_ACC_OUT, series_out, nb * (size_t)c->nout))) return rc;
  return finish(c);
}

int rsf_kstiff_dr_run(rsf_ctx *c, int32_t law, int32_t observable, int64_t n, int32_t d, double *q, double *l, const double *data, int32_t n_groups,
                      const double *lo, const double *hi, const double *chol, double gamma, int32_t stages, double shape, uint64_t seed, int64_t offset,
                      int64_t iter0, int32_t n_iter, int32_t *accepted1, int32_t *accepted2, int32_t *outbox1, int32_t *outbox2, int32_t *stuck,
                      double *trace_q, double *trace_l) {
  RSF_ENTER(c, NEED_MODEL, q && l && data && lo && hi && chol && accepted1 && accepted2 && outbox1 && outbox2 && stuck, "NULL argument");
  int rc;
  if ((rc = check_law(__func__, law, observable))) return rc;
  if (n_iter < 1 || n_iter > RSF_DR_MAX_ITER) return fail(RSF_ERR_INVALID, "rsf_kstiff_dr_run: need 1 <= n_iter <= %d", RSF_DR_MAX_ITER);
  if (!trace_q != !trace_l) return fail(RSF_ERR_INVALID, "rsf_kstiff_dr_run: trace_q and trace_l are both NULL or both given");
  if (stages != 1 && stages != 2) return fail(RSF_ERR_INVALID, "rsf_kstiff_dr_run: stages is 1 or 2");
  if (!good_gamma(gamma) || !std::isfinite(shape) || !(shape > 0.0))
    return fail(RSF_ERR_INVALID, "rsf_kstiff_dr_run: gamma must lie in (0, 1], shape be finite and > 0");
  KDrArgs A{};
  if ((rc = set_chains(__func__, c, n, d, true, n_groups, lo, hi, seed, offset, iter0, n_iter, A))) return rc;
  if ((rc = check_stiffness_box(__func__, d, lo))) return rc;
  if ((rc = check_integrator(__func__, c))) return rc;
  if ((rc = set_factors(__func__, c, d, n_groups, chol, A))) return rc;
  A.gamma = gamma; A.shape = shape; A.stages = stages; A.n_iter = n_iter;
  const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int32_t);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, true), il = s.add(l, nb, true, true);
  const int idata = s.add(data, (size_t)n_groups * c->nout * sizeof(double), true, false);
  const int ia1 = s.add(accepted1, ni, true, true), ia2 = s.add(accepted2, ni, true, true), io1 = s.add(outbox1, ni, true, true);
  const int io2 = s.add(outbox2, ni, true, true), ist = s.add(stuck, ni, true, true);
  const int itq = trace_q ? s.add(trace_q, nb * d * n_iter, false, true) : -1, itl = trace_q ? s.add(trace_l, nb * n_iter, false, true) : -1;
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.l = s.dev<double>(il);
  A.accepted1 = s.dev<int32_t>(ia1); A.accepted2 = s.dev<int32_t>(ia2); A.outbox1 = s.dev<int32_t>(io1); A.outbox2 = s.dev<int32_t>(io2);
  A.stuck = s.dev<int32_t>(ist);
  if (trace_q) { A.tq = s.dev<double>(itq); A.tl = s.dev<double>(itl); }
  // the shared chunking of the float64 tables (c->kc, c->lds_bytes), as rsf_stiff_dr_run
  if ((rc = launch(c, run_fn(c, d, law), grid_for(c, n), c->block, c->lds_bytes, make_consts(c, s.dev<const double>(idata)), A, observable))) return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_kstiff_dr_ssq(rsf_ctx *c, int32_t law, int32_t observable, int64_t n, int32_t d, const double *y, const uint8_t *mask, const double *data,
                      int32_t n_groups, double *ssq) {
  RSF_ENTER(c, NEED_MODEL, y && mask && data && ssq, "NULL argument");
  const double box[2][RSF_KSTIFF_MAX_PARAMS] = {{0.0, 0.0, 0.0, 0.0}, {1.0, 1.0, 1.0, 1.0}};  // the solve takes no box
  int rc;
  if ((rc = check_law(__func__, law, observable))) return rc;
  KDrArgs A{};
  if ((rc = set_chains(__func__, c, n, d, true, n_groups, box[0], box[1], 0, 0, 1, 1, A))) return rc;
  if ((rc = check_integrator(__func__, c))) return rc;
  const size_t nb = (size_t)n * sizeof(double);
  Staged s(c);
  const int iy = s.add(y, nb * d, true, false), im = s.add(mask, (size_t)n, true, false);
  const int idata = s.add(data, (size_t)n_groups * c->nout * sizeof(double), true, false), is = s.add(ssq, nb, true, true);
  if ((rc = s.commit())) return rc;
  if ((rc = launch(c, ssq_fn(c, d, law), grid_for(c, n), c->block, c->lds_bytes, make_consts(c, s.dev<const double>(idata)), A, observable,
                   s.dev<const double>(iy), s.dev<const uint8_t>(im), s.dev<double>(is))))
    return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_kstiff_dr_propose(rsf_ctx *c, int64_t n, int32_t d, const double *q, const double *l, int32_t n_groups, const double *lo, const double *hi,
                          const double *chol, double gamma, int32_t stage, uint64_t seed, int64_t offset, int64_t iter, const uint8_t *pending, double *y,
                          uint8_t *mask) {
  RSF_ENTER(c, NEED_NOTHING, q && l && lo && hi && chol && y && mask, "NULL argument");
  if (stage != 1 && stage != 2) return fail(RSF_ERR_INVALID, "rsf_kstiff_dr_propose: stage is 1 or 2");
  if (stage == 2 && !pending) return fail(RSF_ERR_INVALID, "rsf_kstiff_dr_propose: stage 2 needs pending");
  if (!good_gamma(gamma)) return fail(RSF_ERR_INVALID, "rsf_kstiff_dr_propose: gamma must lie in (0, 1]");
  int rc;
  KDrArgs A{};
  if ((rc = set_chains(__func__, c, n, d, false, n_groups, lo, hi, seed, offset, iter, 1, A))) return rc;
  if ((rc = check_stiffness_box(__func__, d, lo))) return rc;
  if ((rc = set_factors(__func__, c, d, n_groups, chol, A))) return rc;
  A.gamma = gamma; A.stages = stage;
  const size_t nb = (size_t)n * sizeof(double);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, false), il = s.add(l, nb, true, false);
  const int ip = stage == 2 ? s.add(pending, (size_t)n, true, false) : -1;
  const int iy = s.add(y, nb * d, false, true), im = s.add(mask, (size_t)n, false, true);
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.l = s.dev<double>(il);
  if ((rc = launch(c, propose_fn(d), blocks_of(n), kMaxBlock, 0, A, stage == 2 ? s.dev<const uint8_t>(ip) : nullptr, s.dev<double>(iy),
                   s.dev<uint8_t>(im))))
    return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_kstiff_dr_accept(rsf_ctx *c, int64_t n, int32_t d, double *q, double *l, const double *lo, const double *hi, double gamma, int32_t stage,
                         double shape, uint64_t seed, int64_t offset, int64_t iter, const double *y, const uint8_t *mask, const double *ssq, double *l1,
                         uint8_t *pending, int32_t *accepted1, int32_t *accepted2, int32_t *outbox1, int32_t *outbox2, int32_t *stuck) {
  RSF_ENTER(c, NEED_NOTHING, q && l && lo && hi && y && mask && ssq && l1 && pending && accepted1 && accepted2 && outbox1 && outbox2 && stuck,
            "NULL argument");
  if (stage != 1 && stage != 2) return fail(RSF_ERR_INVALID, "rsf_kstiff_dr_accept: stage is 1 or 2");
  if (!good_gamma(gamma) || !std::isfinite(shape) || !(shape > 0.0))
    return fail(RSF_ERR_INVALID, "rsf_kstiff_dr_accept: gamma must lie in (0, 1], shape be finite and > 0");
  int rc;
  KDrArgs A{};
  if ((rc = set_chains(__func__, c, n, d, false, 1, lo, hi, seed, offset, iter, 1, A))) return rc;
  if ((rc = check_stiffness_box(__func__, d, lo))) return rc;
  A.gamma = gamma; A.shape = shape; A.stages = stage;
  const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int32_t);
  const bool first = stage == 1;
  Staged s(c);
  const int iq = s.add(q, nb * d, true, true), il = s.add(l, nb, true, true), iy = s.add(y, nb * d, true, false);
  const int im = s.add(mask, (size_t)n, true, false), is = s.add(ssq, nb, true, false);
  const int il1 = s.add(l1, nb, !first, first), ip = s.add(pending, (size_t)n, !first, first);
  const int ia1 = s.add(accepted1, ni, true, true), ia2 = s.add(accepted2, ni, true, true), io1 = s.add(outbox1, ni, true, true);
  const int io2 = s.add(outbox2, ni, true, true), ist = s.add(stuck, ni, true, true);
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.l = s.dev<double>(il);
  A.accepted1 = s.dev<int32_t>(ia1); A.accepted2 = s.dev<int32_t>(ia2); A.outbox1 = s.dev<int32_t>(io1); A.outbox2 = s.dev<int32_t>(io2);
  A.stuck = s.dev<int32_t>(ist);
  if ((rc = launch(c, accept_fn(d), blocks_of(n), kMaxBlock, 0, A, s.dev<const double>(iy), s.dev<const uint8_t>(im), s.dev<const double>(is),
                   s.dev<double>(il1), s.dev<uint8_t>(ip))))
    return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

}  // extern "C"
