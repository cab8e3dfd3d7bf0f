"""
The specification of the adaptive delayed-rejection run under a state law (tests/law_dr_reference.py) against the quadrature
(CPU, no GPU): 64 chains x 96 iterations at d = 1 on friction data, from qstart = 20 with the Gauss-Newton factor, adapting in the
burn-in's launches as MCMC.sample_law does — the construction whose figures tests/test_gpu_law_dr.py quotes, at a smaller size.
"""
import numpy as np
import pytest

import law_dr_reference as S
import law_reference as R
import observe_cases as OC

Z_MAX = 4.5  # tests/posterior_reference.py's bound on a z score: two-sided normal 6.8e-6


@pytest.mark.parametrize("truth", R.LAWS)
def test_adaptive_specification_keeps_the_quadrature_mean(truth):
    p = OC.friction_problem(truth)
    m, vl, data = p["m"], p["vl"], p["data"]
    fn = S.ssq_fn(m, vl, truth, "mu", data)
    L, cov, ssq = S.gn_factor(m, vl, truth, "mu", [R.BF_TRUTH], data)
    assert L.shape == (1, 1) and ssq > 0 and np.isclose(L[0, 0], 2.38 * np.sqrt(cov[0, 0]))
    n, n_iter, nburn, ipl = 64, 96, 48, 16
    out = S.run(fn, np.full((n, 1), R.BF_TRUTH), *R.BF_BOX, L, n_iter, 0.5 * data.size, gamma=0.2, seed=9, iters_per_launch=ipl,
                adapt_launches=nburn // ipl)
    x = out["trace_q"][nburn:, :, 0]
    means = x.mean(axis=0)
    se = means.std(ddof=1) / np.sqrt(n)
    z = (means.mean() - p["mean"][truth]) / se
    acc = (out["accepted1"].sum() + out["accepted2"].sum()) / (n * n_iter)
    print(f"truth {truth}: pooled mean {means.mean():.4f}, quadrature {p['mean'][truth]:.4f} (SD {p['sd'][truth]:.4f}), pooled SD {x.std():.4f}, "
          f"Laplace SD {np.sqrt(cov[0, 0]):.4f}, SE {se:.2e}, z {z:+.2f}; accepted {acc:.2f}; factor {L[0, 0]:.4f} -> {out['chol'][0, 0]:.4f}")
    assert out["stuck"].sum() == 0 and 0.05 < acc < 0.95
    assert out["chol"][0, 0] != L[0, 0]
    assert abs(z) < Z_MAX
