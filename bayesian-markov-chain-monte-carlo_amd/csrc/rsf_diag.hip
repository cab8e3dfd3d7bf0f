// rsf_diag.hip — convergence diagnostics on the device (include/rsf_diag.h): rsf_diag_partials and the rank-normalised
// rsf_diag_rank_prepare / _partials / _release, whose derived series go through the same partials pass (kernels: rsf_diag.h,
// rsf_diag_rank.h).  The host arithmetic that finishes the partials is rsf_finish.cpp.
#include <climits>
#include <cmath>
#include <algorithm>
#include <vector>

#include "../../include/rsf_diag.h"
#include "rsf_host.h"
#include "rsf_diag.h"
#include "rsf_diag_rank.h"

using namespace rsfk;
using namespace rsfh;

namespace {
auto diag_chain_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return diag_chain_kernel<D>; }); }  // 1 <= d <= RSF_MAX_PARAMS
}  // namespace

extern "C" {

// ---- convergence diagnostics (include/rsf_diag.h) ----------------------------------------------
namespace {
// The lags [lag_begin, lag_end) of a partials call on n draws of C chains and d parameters, and the grid they make: L lags in
// ntiles tiles for each of nbc blocks of chains.  fn: the entry point the messages name.
struct LagGrid { int64_t lag_begin, lag_end, L, nbc, ntiles; };

int check_lags(const char *fn, int64_t n, int64_t C, int32_t d, int64_t lag_begin, int64_t lag_end, LagGrid *g) {
  const int64_t N = n / 2;
  if (lag_begin < 0 || lag_end <= lag_begin || lag_end > N)
    return fail(RSF_ERR_INVALID, "%s: lags [%lld, %lld) are not a non-empty range within [0, %lld)", fn, (long long)lag_begin,
                (long long)lag_end, (long long)N);
  const int64_t L = lag_end - lag_begin;
  *g = {lag_begin, lag_end, L, (C + kDiagBlock - 1) / kDiagBlock, (L + kLagTile - 1) / kLagTile};
  if (g->nbc * d * g->ntiles > INT32_MAX) return fail(RSF_ERR_INVALID, "%s: too many lags for one call; ask for fewer", fn);
  return RSF_OK;
}

// rsf_diag_partials after its checks, on a trace x already in device memory
int diag_partials_dev(rsf_ctx *c, int64_t n, int64_t C, int32_t d, const double *x, int64_t S, const rsfk::DiagCenter &cen,
                      const LagGrid &lg, double *partials) {
  const int64_t N = n / 2, L = lg.L, nbc = lg.nbc;
  const int64_t K = S ? C / S : 0, nbs = S ? std::min<int64_t>(kDiagSuperBlocks, (K + kDiagBlock / 64 - 1) / (kDiagBlock / 64)) : 0;
  // workspace, doubles: mh[2][d][C] | fm[d][C] | fv[d][C] | chain partials[nbc][d][3] | superchain partials[nbs][d][4] |
  // lag partials[nbc][d][L] | sums[d*3 + d*4 + d*L]
  const int64_t nf1 = d * kDiagChainFields, nf2 = d * kDiagSuperFields, nf3 = d * L;
  const int64_t o_fm = 2 * d * C, o_fv = o_fm + d * C, o_p1 = o_fv + d * C, o_p2 = o_p1 + nbc * nf1, o_p3 = o_p2 + nbs * nf2,
                o_sum = o_p3 + nbc * nf3, total = o_sum + nf1 + nf2 + nf3;
  int rc;
  if ((rc = ensure(c->diag, (size_t)total * sizeof(double)))) return rc;
  double *w = (double *)c->diag.p;
  const rsfk::DiagShape sh{n, C, d, N, n - N};
  if ((rc = launch(c, diag_chain_fn(d), (unsigned)nbc, kDiagBlock, 0, sh, x, cen, w, w + o_fm, w + o_fv, w + o_p1))) return rc;
  if (S && (rc = launch(c, diag_super_kernel, (unsigned)nbs, kDiagBlock, 0, C, d, S, cen, w + o_fm, w + o_fv, w + o_p2))) return rc;
  if ((rc = launch(c, diag_lag_kernel, (unsigned)(nbc * d * lg.ntiles), kDiagBlock, 0, sh, x, w, lg.lag_begin, lg.lag_end, w + o_p3))) return rc;
  // the three sums share the grid that covers the longest of them
  const unsigned sum_blocks = (unsigned)((std::max<int64_t>(nf1, std::max(nf2, nf3)) + kDiagBlock - 1) / kDiagBlock);
  if ((rc = sum_in_order(c, nbc, nbc, nf1, w + o_p1, 1.0, w + o_sum, sum_blocks))) return rc;
  if (S && (rc = sum_in_order(c, nbs, nbs, nf2, w + o_p2, 1.0, w + o_sum + nf1, sum_blocks))) return rc;
  if ((rc = sum_in_order(c, nbc, nbc, nf3, w + o_p3, 1.0, w + o_sum + nf1 + nf2, sum_blocks))) return rc;
  std::vector<double> h((size_t)(nf1 + nf2 + nf3), 0.0);
  HIP_TRY(hipMemcpyAsync(h.data(), w + o_sum, sizeof(double) * (size_t)(nf1 + (S ? nf2 : 0)), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(h.data() + nf1 + nf2, w + o_sum + nf1 + nf2, sizeof(double) * (size_t)nf3, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int p = 0; p < d; ++p) {
    double *o = partials + (int64_t)p * (RSF_DIAG_HEAD + L);
    const double *h1 = h.data() + p * kDiagChainFields, *h2 = h.data() + nf1 + p * kDiagSuperFields, *h3 = h.data() + nf1 + nf2 + p * L;
    o[0] = 2.0 * (double)C;
    o[1] = h1[0]; o[2] = h1[1]; o[3] = h1[2];
    o[4] = (double)K;
    for (int f = 0; f < kDiagSuperFields; ++f) o[5 + f] = S ? h2[f] : 0.0;
    for (int64_t j = 0; j < L; ++j) o[RSF_DIAG_HEAD + j] = h3[j];
  }
  return RSF_OK;
}
}  // namespace

int rsf_diag_partials(rsf_ctx *c, int64_t n, int64_t C, int32_t d, const double *trace, int64_t S, const double *center,
                      int64_t lag_begin, int64_t lag_end, double *partials) {
  if (!c || !trace || !center || !partials) return fail(RSF_ERR_INVALID, "rsf_diag_partials: NULL argument");
  if (n < 4 || C < 1 || d < 1 || d > RSF_MAX_PARAMS)
    return fail(RSF_ERR_INVALID, "rsf_diag_partials: need n_iters >= 4, n_chains >= 1, 1 <= n_params <= %d", RSF_MAX_PARAMS);
  if (S < 0 || (S > 0 && C % S)) return fail(RSF_ERR_INVALID, "rsf_diag_partials: chains_per_superchain %lld does not divide %lld chains",
                                             (long long)S, (long long)C);
  if (n > INT64_MAX / 8 / C / d) return fail(RSF_ERR_INVALID, "rsf_diag_partials: trace too large");
  LagGrid lg;
  int rc;
  if ((rc = check_lags("rsf_diag_partials", n, C, d, lag_begin, lag_end, &lg))) return rc;
  rsfk::DiagCenter cen{{0.0, 0.0, 0.0}};
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(center[p])) return fail(RSF_ERR_INVALID, "rsf_diag_partials: center[%d] is not finite", p);
    cen.v[p] = center[p];
  }
  RSF_ENTER(c, NEED_NOTHING);
  const double *dx;
  if ((rc = stage_in(c, SLOT_X, trace, (size_t)(n * C * d) * sizeof(double), &dx))) return rc;
  return diag_partials_dev(c, n, C, d, dx, S, cen, lg, partials);
}

// ---- rank-normalised diagnostics and order statistics (include/rsf_diag.h, rsf_diag_rank_*) ------------------
namespace {
constexpr int64_t kRankMaxDraws = INT64_C(1) << 32;  // 32-bit sort indices

// the rank workspace, carved from c->rank (byte offsets rounded to 256)
struct RankWs {
  double *series;            // [4][A][d]
  uint64_t *keys[2];         // [A]
  uint32_t *idx[2];          // [A + 1] (the spare one holds P during the ranks)
  uint32_t *th;              // [256][ntiles]: tile histograms, then offsets
  uint32_t *tm, *tlast, *tfirst;  // [ntiles]
  uint32_t *hist;            // [8][256] + the non-finite count
  uint32_t *hpart;           // [kRankKeyBlocks][kRankHist]: per-workgroup histograms of rank_key_kernel
  void *part;                // [kRankReduceBlocks] RankArg or 2 doubles
  double *probs, *stats;     // [n_probs], [d][RSF_DIAG_RANK_STATS + n_probs]
};

size_t rank_ws_layout(int64_t A, int d, int np, char *base, RankWs *w) {
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) / 256 * 256; return base ? base + at : nullptr; };  // base NULL: size only
  const int64_t ntiles = (A + kRankTile - 1) / kRankTile;
  w->series = (double *)take((size_t)(4 * A * d) * sizeof(double));
  for (int b = 0; b < 2; ++b) w->keys[b] = (uint64_t *)take((size_t)A * sizeof(uint64_t));
  for (int b = 0; b < 2; ++b) w->idx[b] = (uint32_t *)take((size_t)(A + 1) * sizeof(uint32_t));
  w->th = (uint32_t *)take((size_t)(256 * ntiles) * sizeof(uint32_t));
  w->tm = (uint32_t *)take((size_t)ntiles * sizeof(uint32_t));
  w->tlast = (uint32_t *)take((size_t)ntiles * sizeof(uint32_t));
  w->tfirst = (uint32_t *)take((size_t)ntiles * sizeof(uint32_t));
  w->hist = (uint32_t *)take(kRankHist * sizeof(uint32_t));
  w->hpart = (uint32_t *)take((size_t)kRankKeyBlocks * kRankHist * sizeof(uint32_t));
  w->part = take(kRankReduceBlocks * sizeof(RankArg));
  w->probs = (double *)take((size_t)(np > 0 ? np : 1) * sizeof(double));
  w->stats = (double *)take((size_t)(d * (RSF_DIAG_RANK_STATS + np)) * sizeof(double));
  return o;
}

// Sorts parameter p's keys (of x, or of |x - median| when folded) into keys[*cur] / idx[*cur]; *bad = a non-finite draw
int rank_sort(rsf_ctx *c, RankWs &w, int64_t A, int d, int p, const double *x, bool folded, const double *st, int *cur, bool *bad) {
  const int64_t ntiles = (A + kRankTile - 1) / kRankTile;
  const int nkb = (int)std::min<int64_t>(kRankKeyBlocks, ntiles);
  int rc;
  if ((rc = launch(c, rank_key_kernel, nkb, kRankThreads, 0, A, d, p, x, folded, st, w.keys[0], w.idx[0], w.hpart))) return rc;
  if ((rc = launch(c, rank_hist_kernel, (kRankHist + kRankThreads - 1) / kRankThreads, kRankThreads, 0, nkb, w.hpart, w.hist))) return rc;
  std::vector<uint32_t> h(kRankHist);
  HIP_TRY(hipMemcpyAsync(h.data(), w.hist, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *bad = h[kRankDigits * 256] != 0;
  *cur = 0;
  if (*bad) return RSF_OK;
  for (int g = 0; g < kRankDigits; ++g) {
    bool one = false;  // one bucket holds every key: the pass would not move anything
    for (int b = 0; b < 256; ++b) one = one || (int64_t)h[g * 256 + b] == A;
    if (one) continue;
    const int s = *cur;
    if ((rc = launch(c, rank_upsweep_kernel, (unsigned)ntiles, kRankThreads, 0, A, 8 * g, w.keys[s], w.th, ntiles))) return rc;
    if ((rc = launch(c, rank_offsets_kernel, 256, kRankThreads, 0, w.hist + g * 256, w.th, ntiles))) return rc;
    if ((rc = launch(c, rank_scatter_kernel, (unsigned)ntiles, kRankThreads, 0, A, 8 * g, w.keys[s], w.idx[s], w.keys[1 - s], w.idx[1 - s], w.th, ntiles))) return rc;
    *cur = 1 - s;
  }
  return RSF_OK;
}

// the normal scores of the sorted pairs keys[s] / idx[s] into out (+ p, stride d); idx[1 - s] holds P
int rank_scores(rsf_ctx *c, RankWs &w, const RankShape &rs, int s, double *out) {
  const int64_t ntiles = (rs.A + kRankTile - 1) / kRankTile;
  const uint64_t *k = w.keys[s];
  const uint32_t *ix = w.idx[s];
  uint32_t *P = w.idx[1 - s];
  int rc;
  if ((rc = launch(c, rank_tile_kernel, (unsigned)ntiles, kRankThreads, 0, rs, k, ix, w.tm, w.tlast, w.tfirst))) return rc;
  if ((rc = launch(c, rank_carry_kernel, 1, kRankThreads, 0, ntiles, rs.A, w.tm, w.tlast, w.tfirst))) return rc;
  if ((rc = launch(c, rank_prefix_kernel, (unsigned)ntiles, kRankThreads, 0, rs, k, ix, w.tm, P))) return rc;
  return launch(c, rank_z_kernel, (unsigned)ntiles, kRankThreads, 0, rs, k, ix, w.tlast, w.tfirst, P, out);
}

int rank_grid(int64_t work, int64_t cap) { return (int)std::max<int64_t>(1, std::min<int64_t>(cap, (work + kRankThreads - 1) / kRankThreads)); }
}  // namespace

int rsf_diag_rank_prepare(rsf_ctx *c, int64_t n, int64_t C, int32_t d, const double *trace, int32_t n_probs, const double *probs,
                          double hdi_prob, double *stats, double *series) {
  if (!c || !trace || !stats || (n_probs > 0 && !probs)) return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: NULL argument");
  if (n < 4 || C < 1 || d < 1 || d > RSF_MAX_PARAMS || n_probs < 0)
    return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: need n_iters >= 4, n_chains >= 1, 1 <= n_params <= %d, n_probs >= 0", RSF_MAX_PARAMS);
  if (n >= kRankMaxDraws || C >= kRankMaxDraws || n * C >= kRankMaxDraws)
    return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: n_iters * n_chains must be below 2^32");
  if (const int i = first_bad_prob(n_probs, probs); i >= 0) return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: probs[%d] outside [0, 1]", i);
  const int64_t A = n * C;
  if (!(hdi_prob > 0.0 && hdi_prob < 1.0)) return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: hdi_prob outside (0, 1)");
  const double kd = std::floor(hdi_prob * (double)A);  // ArviZ: int(floor(hdi_prob * n))
  if (kd < 1.0 || kd >= (double)A)
    return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: the HDI of %g of %lld draws spans %g of them; need 1 <= k < n*C", hdi_prob,
                (long long)A, kd);
  const int64_t khdi = (int64_t)kd;
  RSF_ENTER(c, NEED_NOTHING);
  int rc;
  c->rank_d = 0;
  const double *x;
  if ((rc = stage_in(c, SLOT_X, trace, (size_t)(A * d) * sizeof(double), &x))) return rc;
  RankWs w;
  const size_t bytes = rank_ws_layout(A, d, n_probs, nullptr, &w);
  if ((rc = ensure(c->rankws, bytes))) return rc;
  rank_ws_layout(A, d, n_probs, (char *)c->rankws.p, &w);
  const int ns = RSF_DIAG_RANK_STATS + n_probs;
  HIP_TRY(hipMemsetAsync(w.stats, 0, (size_t)(d * ns) * sizeof(double), c->stream));
  if (n_probs) HIP_TRY(hipMemcpyAsync(w.probs, probs, (size_t)n_probs * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const int64_t N = n / 2, stride = A * d;
  std::vector<char> bad((size_t)d, 0);
  for (int p = 0; p < d; ++p) {
    const RankShape rs{A, (n % 2) ? N * C : 0, (n % 2) ? N * C + C : 0, d, p, 2.0 * (double)C * (double)N};
    double *st = w.stats + (int64_t)p * ns;
    int cur;
    bool nonfinite;
    if ((rc = rank_sort(c, w, A, d, p, x, false, st, &cur, &nonfinite))) return rc;
    if (nonfinite) {  // every output of this parameter is NaN
      bad[(size_t)p] = 1;
      if ((rc = launch(c, rank_fill_kernel, rank_grid(A, 4096), kRankThreads, 0, rs, w.series, stride, NAN))) return rc;
      continue;
    }
    const uint64_t *sorted = w.keys[cur];
    if ((rc = launch(c, rank_order_kernel, 1, kRankThreads, 0, sorted, A, n_probs, w.probs, st))) return rc;
    const int nh = rank_grid(A - khdi, kRankReduceBlocks);
    if ((rc = launch(c, rank_hdi_kernel, nh, kRankThreads, 0, sorted, A, khdi, (RankArg *)w.part))) return rc;
    if ((rc = launch(c, rank_hdi_final_kernel, 1, kRankThreads, 0, sorted, A, khdi, nh, (RankArg *)w.part, st))) return rc;
    if ((rc = rank_scores(c, w, rs, cur, w.series))) return rc;                        // bulk: z(x)
    if ((rc = rank_sort(c, w, A, d, p, x, true, st, &cur, &nonfinite))) return rc;    // folded: z(|x - median|)
    if ((rc = rank_scores(c, w, rs, cur, w.series + stride))) return rc;
    if ((rc = launch(c, rank_indicator_kernel, rank_grid(A, 4096), kRankThreads, 0, rs, x, st, w.series + 2 * stride, w.series + 3 * stride))) return rc;
    const int nr = rank_grid(A, kRankReduceBlocks);
    for (int q = 0; q < RSF_DIAG_RANK_SERIES; ++q) {
      if ((rc = launch(c, rank_range_kernel, nr, kRankThreads, 0, rs, w.series + q * stride, (double *)w.part))) return rc;
      if ((rc = launch(c, rank_range_final_kernel, 1, 64, 0, nr, (double *)w.part, st + kStConst + q))) return rc;
    }
  }
  std::vector<double> h((size_t)(d * ns));
  HIP_TRY(hipMemcpyAsync(h.data(), w.stats, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (series)
    HIP_TRY(hipMemcpyAsync(series, w.series, (size_t)(4 * stride) * sizeof(double), host_mem(c) ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int p = 0; p < d; ++p) {
    double *o = stats + (int64_t)p * ns;
    for (int f = 0; f < ns; ++f) o[f] = bad[(size_t)p] ? NAN : h[(size_t)(p * ns + f)];
    o[kStNonFinite] = bad[(size_t)p] ? 1.0 : 0.0;
    if (bad[(size_t)p])
      for (int q = 0; q < RSF_DIAG_RANK_SERIES; ++q) o[kStConst + q] = 0.0;
  }
  c->rank_n = n; c->rank_C = C; c->rank_d = d;
  return RSF_OK;
}

int rsf_diag_rank_partials(rsf_ctx *c, int64_t lag_begin, int64_t lag_end, double *partials) {
  if (!c || !partials) return fail(RSF_ERR_INVALID, "rsf_diag_rank_partials: NULL argument");
  if (!c->rank_d || !c->rankws.p) return fail(RSF_ERR_INVALID, "rsf_diag_rank_partials: no prepared trace (call rsf_diag_rank_prepare first)");
  const int64_t n = c->rank_n, C = c->rank_C;
  const int32_t d = c->rank_d;
  LagGrid lg;
  int rc;
  if ((rc = check_lags("rsf_diag_rank_partials", n, C, d, lag_begin, lag_end, &lg))) return rc;
  RSF_ENTER(c, NEED_NOTHING);
  const rsfk::DiagCenter zero{{0.0, 0.0, 0.0}};
  const double *series = (const double *)c->rankws.p;  // the workspace starts with the series
  for (int q = 0; q < RSF_DIAG_RANK_SERIES; ++q) {
    if ((rc = diag_partials_dev(c, n, C, d, series + q * n * C * d, 0, zero, lg, partials + (int64_t)q * d * (RSF_DIAG_HEAD + lg.L)))) return rc;
  }
  return RSF_OK;
}

int rsf_diag_rank_release(rsf_ctx *c) {
  RSF_ENTER(c, NEED_NOTHING, true, "NULL argument");
  if (c->rankws.p) HIP_TRY(hipStreamSynchronize(c->stream));
  release(c->rankws);
  c->rank_d = 0;
  return RSF_OK;
}

}  // extern "C"
