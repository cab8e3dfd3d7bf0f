"""
CPU tests of the specification of the grid posterior (tests/grid_reference.py) against the closed forms of
tests/posterior_reference.py (SSq = S0 + (q - q0)^T K (q - q0) in a box that truncates; evidence_cases.CLOSED_TRUTH is log I).

Bounds.  log I: the truth is quoted to eleven (d = 1) and seven (d = 3) decimals, and test_evidence_reference.py holds its own
quadratures to 1e-10 and 1e-7 of it; composite Simpson at these node counts is far inside that.  Moments: the reference
(Posterior3, 32 x 32 Gauss-Legendre nodes, a spline of log SSq through 97 points) and the specification on the reference's own
window are two quadratures of one smooth integrand; their distance is bounded by 1e-5 SD for the means and 2e-5 relative for the
variances, five times what a prototype of these rules measured (2e-6 and 5e-6): no Monte Carlo enters.  Draws: the thresholds of
posterior_reference.check (false-alarm probability ~1e-5 per check).
"""
import numpy as np
import pytest

import evidence_cases
import grid_reference as G
import posterior_reference as R

N_DRAWS = 262144
_REFS = {}


def _closed(d):
    if d not in _REFS:
        _REFS[d] = R.closed_reference(d)
    return _REFS[d]


def test_log_integral_d1():
    """4001 Simpson nodes over the whole closed box: the face nodes carry weight (with the samplers' strict box the same rule is
    1.0e-5 short)."""
    _, fn, c = _closed(1)
    x, w = G.simpson(c["lo"][0], c["hi"][0], 4001)
    col, fin, l, _ = G.posterior(fn, [x], [w], c["lo"], c["hi"], c["shape"])
    err = float(fin["log_integral"]) - evidence_cases.CLOSED_TRUTH[1]
    strict = np.where((x > c["lo"][0]) & (x < c["hi"][0]), l, -np.inf)
    cs = G.columns([x], [w], strict, fn(x), float(x[2000]))
    err_strict = float(G.finish([x], [w], G.PLAIN, float(x[2000]), c["shape"], c["lo"], c["hi"], cs["lmax"], cs["fields"])["log_integral"]) - evidence_cases.CLOSED_TRUTH[1]
    print(f"d = 1: log I - truth {err:+.2e} (closed box), {err_strict:+.2e} (strict box)")
    assert abs(err) < 1e-10 and fin["n_neginf"] == 0
    assert -2e-5 < err_strict < -5e-6  # the two face nodes' weight
    # log_evidence carries rsf_evidence_finish's constants
    import math
    want = evidence_cases.CLOSED_TRUTH[1] - math.log(c["hi"][0] - c["lo"][0]) + math.lgamma(c["shape"]) - c["shape"] * math.log(math.pi)
    assert abs(float(fin["log_evidence"]) - want) < 1e-10


def test_log_integral_d3_plain():
    """(1001, 65, 65) Simpson nodes in plain coordinates over the whole box, against a truth quoted to seven decimals"""
    _, fn, c = _closed(3)
    ax = [G.simpson(lo, hi, n) for lo, hi, n in zip(c["lo"], c["hi"], (1001, 65, 65))]
    _, fin, _, _ = G.posterior(fn, [a[0] for a in ax], [a[1] for a in ax], c["lo"], c["hi"], c["shape"])
    err = float(fin["log_integral"]) - evidence_cases.CLOSED_TRUTH[3]
    print(f"d = 3 plain: log I - truth {err:+.2e}")
    assert abs(err) < 1e-7


def _product_grid(ref, c, n0, n12, rule):
    ax = [G.simpson(ref.plo, ref.phi, n0)] + [rule(c["lo"][p], c["hi"][p], n12) for p in (1, 2)]
    return [a[0] for a in ax], [a[1] for a in ax]


def test_moments_d3_product():
    """(2001, 32 GL, 32 GL) in product coordinates on the reference's window: means and variances of Dc, a, b and Dc a"""
    ref, fn, c = _closed(3)
    x, w = _product_grid(ref, c, 2001, 32, G.gauss_legendre)
    _, fin, _, _ = G.posterior(fn, x, w, c["lo"], c["hi"], c["shape"], G.PRODUCT)
    got = {"Dc": (fin["mean"][0], fin["cov"][0, 0]), "a": (fin["mean"][1], fin["cov"][1, 1]), "b": (fin["mean"][2], fin["cov"][2, 2]),
           "Dc*a": (fin["x0_mean"], fin["x0_var"]), "sigma2": (fin["std2_mean"], fin["std2_var"])}
    worst_m = worst_v = 0.0
    for name, (m, v) in got.items():
        mg = ref.marg[name]
        dm, dv = abs(float(m) - mg.mean) / mg.sd, abs(float(v) - mg.var) / mg.var
        print(f"{name}: mean {float(m):.10g} (reference {mg.mean:.10g}, {dm:.2e} SD), variance {float(v):.10g} ({dv:.2e} relative)")
        worst_m, worst_v = max(worst_m, dm), max(worst_v, dv)
    assert worst_m < 1e-5 and worst_v < 2e-5
    # the covariance of Dc and a by the definition, from the node weights
    q = G.nodes(x, G.PRODUCT)
    s = fn(*q.T)
    l = G.log_density(q, s, c["shape"], c["lo"], c["hi"], G.PRODUCT)
    W = (w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]).ravel(order="F").astype(G.LD) * np.exp((l - l.max()).astype(G.LD))
    W /= W.sum()
    m = (W[:, None] * q).sum(axis=0)
    cov = ((q - m) * W[:, None]).T @ (q - m)
    np.testing.assert_allclose(np.asarray(fin["mean"], dtype=np.float64), np.asarray(m, dtype=np.float64), rtol=1e-12)
    np.testing.assert_allclose(np.asarray(fin["cov"], dtype=np.float64), np.asarray(cov, dtype=np.float64), rtol=1e-9, atol=1e-14)


def _draws(d, n12, seed):
    ref, fn, c = _closed(d)
    if d == 1:
        x, w = G.simpson(c["lo"][0], c["hi"][0], 4001)
        x, w, coords = [x], [w], G.PLAIN
    else:
        (x, w), coords = _product_grid(ref, c, 2001, n12, G.simpson), G.PRODUCT
    col, fin, _, _ = G.posterior(fn, x, w, c["lo"], c["hi"], c["shape"], coords, dtype=np.float64)
    out = G.draw(x, coords, col["cum0"], fin.get("cum1"), fin.get("cum2"), seed, 0, N_DRAWS)
    q = out["q"]
    std2 = R.draw_std2(np.random.default_rng(seed), fn(*q.T), c["shape"])
    fails = []
    zmax, kmax = R.check(f"d = {d}, {n12} nodes, seed {seed}", ref, q, std2, fails)
    print(f"d = {d}, {n12} nodes, seed {seed}: largest |z| {zmax:.2f}, largest sqrt(C) D {kmax:.2f}")
    return fails, zmax


def test_draws_d1():
    fails, _ = _draws(1, 0, 1)
    assert not fails, fails


@pytest.mark.parametrize("seed", [1, 2])
def test_draws_d3(seed):
    """65 nodes on axes 1 and 2, the default"""
    fails, _ = _draws(3, 65, seed)
    assert not fails, fails


def test_draws_d3_33_nodes_show_the_trapezoid_cdf():
    """33 nodes on axes 1 and 2: the piecewise-linear density of the trapezoid CDF shows at 262 144 draws — why the default is 65"""
    fails, zmax = _draws(3, 33, 1)
    assert fails and zmax > R.Z_MAX


def test_inversion_rules():
    """the cell is the largest k <= n - 2 with F[k] <= u; a cell without mass gives its lower node; a tie goes to the lower node"""
    x = np.array([0.0, 1.0, 2.0, 4.0])
    F = np.array([0.0, 0.25, 0.25, 1.0])
    v, k, node = G.invert(F, x, np.array([0.25, 0.125, 1.0, 0.625, 1e-300]))
    assert k.tolist() == [2, 0, 2, 2, 0]
    np.testing.assert_array_equal(v, [2.0, 0.5, 4.0, 3.0, 4e-300])
    assert node.tolist() == [2, 0, 3, 2, 0]  # 0.5 and 3.0 lie midway: the lower node
    v, k, _ = G.invert(np.array([0.0, 0.0, 1.0]), np.array([1.0, 2.0, 3.0]), np.array([0.5]))
    assert k.tolist() == [1] and v.tolist() == [2.5]


def test_every_node_without_density():
    x, w = G.simpson(0.0, 1.0, 5)
    col = G.columns([x], [w], np.full(5, -np.inf), np.full(5, np.nan), 0.5)
    assert col["lmax"] == -np.inf and not col["fields"][:, :5].any() and col["fields"][0, 5] == 5
    fin = G.finish([x], [w], G.PLAIN, 0.5, 3.0, [0.0], [1.0], col["lmax"], col["fields"])
    assert fin["log_integral"] == -np.inf and fin["n_neginf"] == 5 and np.isnan(fin["log_evidence"])
