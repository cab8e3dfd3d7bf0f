"""
GPU tests of the exact posterior of a state-law model on a tensor grid in the coordinates of a fit (include/rsf_law_grid.h:
rsf_law_logtarget / rsf_law_grid_moments; Engine.law_logtarget / law_grid_moments / law_grid_posterior / law_evidence;
MCMC.quadrature_law / bayes_factor_laws; PosteriorPool.law_evidence) against its specification (tests/law_grid_reference.py):
  1. the kernel's corners: the node formation, the box, ssq bit for bit rsf_law_observe's (and rsf_law_forward's), the point mode;
  2. the moments and the z-grid reductions on the GPU's own l against the long-double sums;
  3. d = 1 with the identity map on the fine nodes of MCMC.quadrature() under the slip law: the split path's ssq, its evidence;
  4. end to end at d = 3 on both friction problems; 5. the Bayes factor; 6. the samplers against the exact posterior;
  7. the error codes through ctypes.

Bounds.  q_out: 4 ulp of the long-double formation (one rounding of phi and the device exponential; identity coordinates: one
rounding).  ssq: bits.  l against -shape log ssq + J: 2 ulp of |l|, tests/test_gpu_grid.py's for the same comparison (J the
specification's sum of the logged phi_p; the kernel's is the sum of log q_p, 1e-16 of it away).  The point mode's l and ssq on q_out: bits.
Sums: 1e-12 of the scale of each, tests/test_gpu_grid.py's.  End to end: 250 x 1e-9 on log_evidence (shape = N / 2 = 250 times the family's
1e-9 cap on the relative error of SSq), 1e-6 relative on mean and SD, edge_mass below 1e-8, evidence_spread below 10 x the
specification's own (tests/test_law_grid_reference.py measures it: 2.19e-6 ageing truth, 9.50e-6 slip truth).
"""
import numpy as np
import pytest

import law_fit_reference as LF
import law_grid_reference as LG
import law_reference as R
import observe_cases as OC
import posterior_reference as PR

pytestmark = pytest.mark.gpu

LD = np.longdouble
TOL = 1e-12
SPREAD_SPEC = {"aging": 2.19e-6, "slip": 9.50e-6}  # the specification's evidence_spread on E2E_N, E2E_WINDOW (test_law_grid_reference.py)
LO3, HI3 = LF.BOX[3]
# a fit-like map about (20, 0.011, 0.014): SDs (0.25, 1.1e-4, 9.4e-5), corr(a, b) = 0.93, corr(Dc, a) = -0.82, corr(Dc, b) = -0.7
POINT = np.array([20.0, 0.011, 0.014])
SD = np.array([0.25, 1.1e-4, 9.4e-5])
CORR = np.array([[1.0, -0.82, -0.70], [-0.82, 1.0, 0.93], [-0.70, 0.93, 1.0]])
COV = CORR * SD[:, None] * SD[None, :]


def _model(pkg, nsteps=500, substeps=1, history="step", **attrs):
    m = pkg.RateStateModel(number_time_steps=nsteps)
    m.substeps = substeps
    if history != "builtin":
        m.loading = R.HISTORIES[history]
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def _observe(eng, law, obs, q, data):
    ab = [np.ascontiguousarray(q[:, p]) for p in (1, 2)] if q.shape[1] == 3 else [None, None]
    return np.asarray(eng.law_observe(law, obs, np.ascontiguousarray(q[:, 0]), ab[0], ab[1], data=data, want_ssq=True, want_series=False)[0])


def _data(eng, law, obs):
    """the series of `obs` at POINT under `law` plus 5 % of its excursion (its size for the acceleration) N(0, 1)"""
    s = np.asarray(eng.law_observe(law, obs, POINT[:1], POINT[1:2], POINT[2:3], want_series=True)[1])[:, 0]
    return s + 0.05 * np.abs(s - s[0]).max() * np.random.default_rng(5).standard_normal(s.size)


# name: (d, n, window_sd, law, observable, model kw, log_coords, first, scale of the factor)
CORNERS = {
    "partial_wave": (3, (5, 3, 3), 3.0, "aging", "mu", {}, (), 0, 1.0),
    "straddle": (3, (67, 3, 3), 4.0, "slip", "mu", {}, (), 0, 1.0),
    "straddle_log_a_first": (3, (67, 3, 3), 4.0, "aging", "acc", {}, (0, 1), 1, 1.0),
    # the factor 40 x: +- 3.7 "SD" of Dc is +- 37 and a moves by 3.6e-3 per unit of z0, so that only a band about the middle of each
    # column of 257 nodes is inside the box: whole waves outside next to waves with lanes inside in one workgroup
    "across_faces": (3, (257, 3, 3), 3.7, "slip", "velocity", {}, (), 0, 40.0),
    "d1": (1, (193,), 6.0, "slip", "theta", {}, (), 0, 1.0),
    "d1_log": (1, (67,), 6.0, "aging", "mu", {}, (0,), 0, 1.0),
    "undamped": (3, (67, 3, 3), 4.0, "aging", "mu", dict(RadiationDamping=False), (), 2, 1.0),
    "k1zero_b_first": (3, (33, 5, 3), 4.0, "slip", "acc", dict(k1=0.0), (), 2, 1.0),
    "two_chunks": (3, (67, 3, 3), 4.0, "slip", "mu", dict(nsteps=900, substeps=4), (), 0, 1.0),
    "substeps2": (3, (67, 3, 3), 4.0, "aging", "theta", dict(substeps=2), (), 0, 1.0),
    "hold_history": (3, (67, 3, 3), 4.0, "aging", "velocity", dict(history="hold"), (2,), 0, 1.0),
    "builtin_forward": (3, (67, 3, 3), 4.0, "aging", "acc", dict(history="builtin"), (), 0, 1.0),
}


@pytest.mark.parametrize("name", CORNERS)
def test_kernel_corners(pkg, name):
    d, n, win, law, obs, kw, logged, first, scale = CORNERS[name]
    m, L, tr, perm = LG.factor(POINT[:d], scale ** 2 * COV[:d, :d], logged, first)
    z, w = LG.axes(n, win)
    lo, hi = (LO3, HI3) if d == 3 else (LO3[:1], HI3[:1])
    with pkg.Engine(mem="host") as eng:
        eng.set_model(_model(pkg, **kw), kw.get("substeps", 1))
        data = _data(eng, law, obs)
        shape = 0.5 * data.size
        l, ssq, q = (np.asarray(v) for v in eng.law_logtarget(law, obs, data, lo, hi, z=z, m=m, L=L, tr=tr, perm=perm, want_q=True))
        # the formation: 4 ulp of long double's, and inside or outside the box as the specification's float64 nodes are
        qs, jac, _ = LG.nodes(z, m, L, tr, perm)
        qx = LG.nodes(z, m, L, tr, perm, dtype=LD)[0]
        ulp = float((np.abs(q.astype(LD) - qx) / np.spacing(np.abs(qx).astype(np.float64))).max())
        inb = LG.in_box(q, lo, hi)
        # a node whose long-double value lies within 4 ulp of a face may fall on either side: none does here
        near = (np.abs(qx - lo) <= 4 * np.spacing(lo)) | (np.abs(qx - hi) <= 4 * np.spacing(hi))
        assert not near.any()
        np.testing.assert_array_equal(inb, LG.in_box(qs, lo, hi))
        np.testing.assert_array_equal(inb, ((qx >= lo) & (qx <= hi)).all(axis=1))
        print(f"{name}: {len(q)} nodes, {int(inb.sum())} inside; q_out against long double {ulp:.2f} ulp")
        assert ulp <= 4.0
        if name == "across_faces":  # whole waves outside beside waves inside, in one workgroup
            waves = inb[:256 * (len(q) // 256)].reshape(-1, 4, 64).any(axis=2)
            assert (waves.any(axis=1) & ~waves.all(axis=1)).any()
        else:
            assert inb.all()
        # outside: -inf and NaN; inside: rsf_law_observe's bits
        np.testing.assert_array_equal(np.isnan(ssq), ~inb)
        assert (l[~inb] == -np.inf).all() and np.isfinite(l[inb]).all()
        want = _observe(eng, law, obs, np.ascontiguousarray(q[inb]), data)
        np.testing.assert_array_equal(_bits(ssq[inb]), _bits(want))
        if law == "aging" and obs == "acc":
            ab = [np.ascontiguousarray(q[inb, p]) for p in (1, 2)]
            fw = np.asarray(eng.law_forward(law, np.ascontiguousarray(q[inb, 0]), ab[0], ab[1], data=data, want_ssq=True, want_acc=False)[0])
            np.testing.assert_array_equal(_bits(ssq[inb]), _bits(fw))
        # l is the rule applied to the kernel's own ssq and the specification's Jacobian
        rule = LG.log_target(ssq, jac, inb, shape)
        assert (np.abs(l[inb] - rule[inb]) <= 2 * np.spacing(np.abs(l[inb]))).all()
        # the point mode on q_out
        lp, sp = (np.asarray(v) for v in eng.law_logtarget(law, obs, data, lo, hi, theta=q, logg=np.zeros(len(q)), tr=tr, perm=perm))
        np.testing.assert_array_equal(_bits(sp), _bits(ssq))
        np.testing.assert_array_equal(_bits(lp), _bits(l))
        # logg is subtracted; without logg nothing is
        g = np.linspace(-3.0, 5.0, len(q))
        lg = np.asarray(eng.law_logtarget(law, obs, data, lo, hi, theta=q, logg=g, tr=tr, perm=perm)[0])
        np.testing.assert_array_equal(_bits(lg[inb]), _bits(lp[inb] - g[inb]))
        l0 = np.asarray(eng.law_logtarget(law, obs, data, lo, hi, theta=q, tr=tr, perm=perm)[0])
        np.testing.assert_array_equal(_bits(l0), _bits(lp))


@pytest.mark.parametrize("d", (1, 3))
def test_one_point(pkg, d):
    """N = 1: one lane of one wave"""
    with pkg.Engine(mem="host") as eng:
        eng.set_model(_model(pkg), 1)
        data = _data(eng, "slip", "mu")
        q = POINT[None, :d] * 1.01
        l, ssq, qo = (np.asarray(v) for v in eng.law_logtarget("slip", "mu", data, LO3[:d], HI3[:d], theta=q, want_q=True))
        np.testing.assert_array_equal(qo, q)
        np.testing.assert_array_equal(_bits(ssq), _bits(_observe(eng, "slip", "mu", q, data)))
        assert abs(l[0] + 0.5 * data.size * np.log(ssq[0])) <= 2 * np.spacing(abs(l[0]))
        out = np.asarray(eng.law_logtarget("slip", "mu", data, LO3[:d], HI3[:d], theta=q * 100.0)[0])
        assert out[0] == -np.inf


def _scaled(name, got, want, scale):
    got, want, scale = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD), np.broadcast_to(np.asarray(scale, dtype=LD), np.shape(want))
    err = np.abs(got - want)
    bad = err > TOL * scale + np.finfo(np.float64).tiny
    assert not bad.any(), f"{name}: {int(bad.sum())} entries beyond {TOL} scaled, worst {float((err / np.where(scale > 0, scale, 1)).max()):.2e}"
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


@pytest.mark.parametrize("d,n,logged,first,scale", [(3, (67, 5, 3), (), 0, 1.0), (3, (261, 3, 5), (0, 1), 1, 30.0), (1, (67,), (0,), 0, 1.0)])
def test_moments_and_reductions(pkg, d, n, logged, first, scale):
    """the GPU's own l and ssq summed in long double: rsf_law_grid_moments' totals and columns, and rsf_grid_columns / _finish on the
    z-grid (lmax, the integral, the axes' masses); (261, 3, 5) at 30 x the factor has nodes outside the box and two rounds of the
    256 threads per column"""
    m, L, tr, perm = LG.factor(POINT[:d], scale ** 2 * COV[:d, :d], logged, first)
    z, w = LG.axes(n, 4.0)
    lo, hi = LO3[:d], HI3[:d]
    with pkg.Engine(mem="host") as eng:
        eng.set_model(_model(pkg), 1)
        data = _data(eng, "aging", "mu")
        shape = 0.5 * data.size
        l, ssq, q = (np.asarray(v) for v in eng.law_logtarget("aging", "mu", data, lo, hi, z=z, m=m, L=L, tr=tr, perm=perm, want_q=True))
        col = eng.grid_columns(z, w, l, ssq, center=0.0)
        fin = eng.grid_finish(z, w, lo, hi, shape, col["lmax"], col["fields"], 0.0)
        center = POINT[:d] * 1.001
        total, fields = eng.law_grid_moments(z, w, m, L, tr, perm, l, ssq, col["lmax"], center, return_fields=True)
        again = eng.law_grid_moments(z, w, m, L, tr, perm, l, ssq, col["lmax"], center)
    zs = LG.z_sums(z, w, l)
    assert col["lmax"] == zs["lmax"] and fin["n_neginf"] == zs["n_neginf"] == int((l == -np.inf).sum())
    if scale > 1:
        assert zs["n_neginf"] > 0
    want = LG.moments(w, l, ssq, q, zs["lmax"], center)
    sp = np.zeros(3)
    sp[:d] = np.abs(q - center).max(axis=0)
    s0, sq = want[0], np.nanmax(ssq)
    scales = [s0] + [s0 * sp[p] for p in range(3)] + [s0 * sp[p] * sp[r] for p, r in LG.PAIRS] + [s0 * sq, s0 * sq * sq]
    worst = max(_scaled(k, total[i], want[i], scales[i]) for i, k in enumerate(pkg._abi.LAW_GRID_FIELDS))
    np.testing.assert_array_equal(_bits(total), _bits(again))
    # the totals are the columns added in index order
    acc = np.zeros(LG.FIELDS)
    for row in fields:
        acc = acc + row
    np.testing.assert_array_equal(_bits(acc), _bits(total))
    worst = max(worst, _scaled("Z", fin["Z"], zs["Z"], zs["Z"]), _scaled("log_integral", fin["log_integral"], zs["log_integral"], abs(zs["log_integral"])))
    mass = [w[0] * col["m0"] / fin["Z"]] + [fin[f"mass{p}"] for p in range(1, d)]
    for p in range(d):
        worst = max(worst, _scaled(f"mass{p}", mass[p], zs["mass"][p], 1.0))
    print(f"d = {d} n = {n}: {zs['n_neginf']} nodes without density, worst scaled error {worst:.2e}")


def _friction(pkg, truth, law=None, d=3):
    p = OC.friction_problem(truth)
    model = _model(pkg, observable="mu", state_law=law or truth)
    model.loading = p["vl"]
    if d == 1:
        return p, model, pkg.MCMC(model, p["data"], R.BF_TRUTH, ["Uniform", *R.BF_BOX], 40.0, nsamples=10, verbose=False)
    pri = [["Uniform", float(LO3[k]), float(HI3[k])] for k in range(3)]
    return p, model, pkg.MCMC(model, p["data"], R.BF_TRUTH, pri, np.array([25.0, 0.0115, 0.0145]), nsamples=10, verbose=False)


def test_d1_identity_map_is_the_split_quadrature(pkg):
    """the fine nodes of MCMC.quadrature() under the slip law on friction data, as a z-axis under m = 0, L = 1: q = 0 + 1 x is x.
    ssq: the split path's (law_ssq_fn -> rsf_law_observe) bits.  The evidence after the same reductions (rsf_grid_columns,
    rsf_grid_finish): EQUAL where l is formed from the fused ssq as the split path forms it (-shape log SSq by NumPy on the host);
    the fused kernel's own l takes the device's logarithm instead, which may differ from NumPy's in the last bit of an l — through
    the same reductions within 1e-12 relative (measured: the same digits, 2597.169506156628)"""
    p, model, mc = _friction(pkg, "slip", d=1)
    res = mc.quadrature(mem="host")
    try:
        eng, x, w = res.engine, res.x, res.w
        l, ssq, q = (np.asarray(v) for v in eng.law_logtarget("slip", "mu", p["data"], res.lo, res.hi, z=x, m=[0.0], L=[[1.0]], want_q=True))
        np.testing.assert_array_equal(q[:, 0], x[0])
        split = eng.law_ssq_fn("slip", p["data"], "mu")(x[0][:, None])
        np.testing.assert_array_equal(_bits(ssq), _bits(split))

        def reduce(lv):
            col = eng.grid_columns(x, w, lv, ssq)
            return eng.grid_finish(x, w, res.lo, res.hi, res.shape, col["lmax"], col["fields"], col["center"])

        same = reduce(-res.shape * np.log(ssq))  # the split path's rule on the fused kernel's ssq
        assert same["log_evidence"] == res.log_evidence and same["mean"][0] == res.mean[0] and same["cov"][0, 0] == res.cov[0, 0]
        fin = reduce(l)
        print(f"d = 1, {x[0].size} nodes: log evidence {fin['log_evidence']!r} from the fused l, {same['log_evidence']!r} from the host's rule on the fused "
              f"ssq, the split path's {res.log_evidence!r}; l differs from the host's rule in {int((l != -res.shape * np.log(ssq)).sum())} nodes")
        assert abs(fin["log_evidence"] - res.log_evidence) <= 1e-12 * abs(res.log_evidence)
        assert abs(fin["mean"][0] - res.mean[0]) <= 1e-12 * res.mean[0]
    finally:
        res.engine.close()


E2E = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in E2E.values():
        r.engine.close()
    E2E.clear()


def _e2e(pkg, truth, first):
    """Engine.law_grid_posterior on the specification's grid: its fit's point and the factor of its covariance"""
    if (truth, first) not in E2E:
        p, model, _ = _friction(pkg, truth)
        _, _, _, _, point, cov = LG.fit_map(truth, truth)
        eng = pkg.Engine(mem="host")
        eng.set_model(model, 1)
        E2E[truth, first] = eng.law_grid_posterior(truth, "mu", p["data"], LO3, HI3, point, np.linalg.cholesky(cov), first=first, n=LG.E2E_N,
                                                   window_sd=LG.E2E_WINDOW)
    return E2E[truth, first]


@pytest.mark.parametrize("truth", R.LAWS)
def test_end_to_end(pkg, truth):
    spec = LG.e2e(truth, truth)
    res = [_e2e(pkg, truth, f) for f in ("Dc", "a", "b")]
    got = res[0]
    err = abs(got.log_evidence - float(spec["log_evidence"]))
    em = np.abs(got.mean / np.asarray(spec["mean"], dtype=np.float64) - 1).max()
    es = np.abs(np.sqrt(np.diag(got.cov)) / np.asarray(spec["sd"], dtype=np.float64) - 1).max()
    spread = max(r.log_evidence for r in res) - min(r.log_evidence for r in res)
    print(f"truth {truth}: log_evidence {got.log_evidence!r} against the specification's {float(spec['log_evidence'])!r}: {err:.2e}; mean {em:.2e}, "
          f"SD {es:.2e} relative; edge_mass {got.edge_mass:.3e} (specification {spec['edge_mass']:.3e}); n_neginf {got.n_neginf}; evidence_spread "
          f"{spread:.3e} (specification {SPREAD_SPEC[truth]:.3e}); windows {got.windows}, {got.n_solves} solves")
    assert got.n == LG.E2E_N and got.windows == (LG.E2E_WINDOW,) * 3 and got.n_neginf == spec["n_neginf"] == 0
    assert err <= 250 * 1e-9
    assert em <= 1e-6 and es <= 1e-6
    assert abs(got.std2_mean / float(spec["std2_mean"]) - 1) <= 1e-6
    assert got.edge_mass < 1e-8
    assert spread <= 10 * SPREAD_SPEC[truth]
    # the marginal of each grid's first parameter carries that parameter's mean and SD
    for k, r in enumerate(res):
        x, f, F = r.marginal()
        mean = float((0.5 * (x[1:] * f[1:] + x[:-1] * f[:-1]) * np.diff(x)).sum())
        assert r.first == k and abs(mean / got.mean[k] - 1) <= 1e-4 and F[0] == 0.0 and abs(F[-1] - 1) <= 1e-12
        qs = r.quantiles((0.025, 0.5, 0.975))
        # rsf_grid_cdf interpolates each column's CDF linearly between nodes h = 0.375 SD apart: h^2 / 8 max|f'| = 4.3e-3
        np.testing.assert_allclose(r.cdf(qs), (0.025, 0.5, 0.975), atol=1e-2)


def test_bayes_factor_laws(pkg):
    """the true law on both data sets, |log BF| > 20 (the specification: -547.9 ageing truth, +584.9 slip truth; the law the data
    contradict is fitted onto a face of the box, its grid is cut and its evidence approximate)"""
    for truth in R.LAWS:
        p, model, mc = _friction(pkg, truth)
        out = mc.bayes_factor_laws(n=LG.E2E_N, window_sd=LG.E2E_WINDOW, n_starts=8, mem="host")
        try:
            bf = out["log_bayes_factor"]
            lap = out[truth].fit.laplace(lo=LO3, hi=HI3)["log_evidence"]
            print(f"truth {truth}: log BF (slip - ageing) {bf:+.3f}; " + "; ".join(
                f"{law}: log_evidence {out[law].log_evidence:.4f} n {out[law].n} windows {out[law].windows} n_neginf {out[law].n_neginf} edge {out[law].edge_mass:.2e}"
                for law in R.LAWS) + f"; FitResult.laplace() under the true law {lap:.4f}: {lap - out[truth].log_evidence:+.2e} off the exact")
            assert model.state_law == truth
            assert abs(bf) > 20 and (bf > 0) == (truth == "slip")
        finally:
            for law in R.LAWS:
                out[law].engine.close()


def _marginal_ref(grids):
    """posterior_reference.check's reference from the grids' axis-0 marginals"""
    class Ref:
        names, marg = tuple(grids), {}
    for name, g in grids.items():
        x, mass = g._q0(g.z[0]), g.mass[0]
        mean, var, kurt = PR._moments(x, mass / mass.sum())
        Ref.marg[name] = PR.Marginal(mean, var, kurt, x, g.marginal()[2])
    return Ref


def test_samplers_keep_the_exact_posterior(pkg):
    """256 sample_law chains at d = 3 from the fit's point under the true law (slip), their last states held to the grids' marginals of
    Dc, a and b by posterior_reference.check; then exact draws of the grid by the same rule, and PosteriorPool.law_evidence on
    LawGridPosterior.pool(16384) against log_evidence by test_gpu_evidence.py's rule: within Z_MAX of its own re"""
    truth = "slip"
    p, model, mc = _friction(pkg, truth)
    res = mc.quadrature_law(n=(65, 33, 33), window_sd=8.0, n_starts=8, marginals=("Dc", "a", "b"), mem="host")
    try:
        ref = _marginal_ref(res.grids)
        print(f"quadrature_law: log_evidence {res.log_evidence!r}, evidence_spread {res.evidence_spread:.2e}, edge_mass {res.edge_mass:.2e}, {res.n_solves} solves")
        fails = []
        q, std2 = res.draw(256, seed=3)
        PR.check("exact draws", ref, q, std2, fails)
        point = res.fit.q[res.fit.best()]
        pool = mc.sample_law(256, 640, start=np.tile(point, (256, 1)), seed=11, mem="host")
        PR.check("sample_law", ref, np.asarray(pool.samples)[-1], np.asarray(pool.std2)[-1], fails)
        assert not fails, fails
    finally:
        res.engine.close()
    # the pool of the default grid, 65 nodes per axis: a draw inverts piecewise-linear tables, so the pool is the posterior as well as
    # the nodes resolve it (on the (65, 33, 33) grid above the same estimate lay 4.0 re below the exact value: -3.16e-3, re 7.87e-4)
    fine = mc.quadrature_law(n_starts=8, mem="host")
    try:
        gp = fine.pool(16384, seed=5)
        ev = gp.law_evidence(model, p["data"], LO3, HI3, engine=fine.engine)
        err = ev["log_evidence"] - fine.log_evidence
        # the specification on the same draws (tests/test_gpu_evidence.py's rule): the pool's rows split as a flat pool splits, the
        # library's proposal draws are the normals of (seed 0, chain j, iteration 0), and the draws are independent (ess_factor 1)
        flat = np.asarray(gp.samples).reshape(-1, 3)
        theta, _, _ = fine.engine.evidence_propose(ev["mean"], ev["chol"], LO3, HI3, ev["n2"], seed=0)
        zn = np.linalg.solve(ev["chol"], (np.asarray(theta) - ev["mean"]).T).T
        import evidence_reference as ER
        import law_dr_reference as LDR
        want = ER.evidence(flat, LDR.ssq_fn(p["m"], p["vl"], "slip", "mu", p["data"]), LO3, HI3, fine.shape, zn)
        print(f"law_evidence on pool(16384) of the {fine.n} grid: {ev['log_evidence']!r} against {fine.log_evidence!r}: {err:+.2e}; re {ev['re']:.3e} "
              f"(ess_factor {ev['ess_factor']:.3f}), the specification's on the same draws {float(want['re']):.3e} (z {err / float(want['re']):+.2f}), its estimate "
              f"{float(want['log_evidence'])!r}; law {ev['law']} observable {ev['observable']}")
        assert ev["converged"] and ev["law"] == "slip" and ev["observable"] == "mu" and ev["n1"] == ev["n2"] == 8192
        assert abs(err) < PR.Z_MAX * float(want["re"])
        # the same estimator on the same draws: every l within shape x 1e-9 (the cap on SSq), the iteration stopped within 100 x its
        # tolerance of its fixed point on either side
        assert abs(ev["log_evidence"] - float(want["log_evidence"])) <= 250 * 1e-9 + 100 * pkg._abi.EVIDENCE_RTOL
    finally:
        fine.engine.close()


def test_error_codes(pkg):
    P = lambda x: x.ctypes.data
    i32 = lambda v: np.asarray(v, dtype=np.int32).ctypes.data_as(pkg._abi._I32P)
    dp = lambda v: np.atleast_1d(np.asarray(v, dtype=np.float64)).ctypes.data_as(pkg._abi._DP)
    n = np.array([5, 3, 3], np.int32)
    z = np.concatenate([np.linspace(-1, 1, 5), np.linspace(-1, 1, 3), np.linspace(-1, 1, 3)])
    w = np.ones_like(z)
    N = 45
    m, L = POINT.copy(), np.array([0.25, 0.0, 1e-4, 0.0, 0.0, 1e-4])
    data, l, ssq, q, th = np.cos(np.linspace(0.0, 3.0, 500)) + 2.0, np.zeros(N), np.ones(N), np.zeros((N, 3)), np.tile(POINT, (N, 1))
    with pkg.Engine(mem="host") as eng:
        lib, ctx = eng.lib, eng._ctx
        target = lambda: [ctx, 1, 1, 3, i32(n), dp(z), dp(m), dp(L), i32([0, 0, 0]), i32([0, 1, 2]), 0, None, None, P(data), 250.0, dp(LO3), dp(HI3), P(l), P(ssq), P(q)]
        moments = lambda: [ctx, 3, i32(n), dp(z), dp(w), dp(m), dp(L), i32([0, 0, 0]), i32([0, 1, 2]), P(l), P(ssq), 0.0, dp(POINT), None, dp(np.zeros(12))]
        name = b"rsf_law_logtarget"
        assert lib.rsf_law_logtarget(*target()) == -3 and name in lib.rsf_last_error()  # no model
        eng.set_model(_model(pkg), 1)
        assert lib.rsf_law_logtarget(*target()) == 0
        assert lib.rsf_law_grid_moments(*moments()) == 0
        bad_target = ((1, -1), (1, 2), (2, -1), (2, 4), (3, 2), (3, 0), (4, None), (4, i32([1, 3, 3])), (5, None), (5, dp(z[::-1].copy())), (6, None),
                      (6, dp([np.nan, 0.011, 0.014])), (7, None), (7, dp([0.0, 0.0, 1e-4, 0.0, 0.0, 1e-4])), (7, dp([0.25, np.inf, 1e-4, 0.0, 0.0, 1e-4])),
                      (8, None), (9, None), (9, i32([0, 0, 2])), (9, i32([0, 1, 3])), (13, None), (14, 0.0), (14, np.nan), (15, None),
                      (16, None), (15, dp([60.0, 0.009, 0.012])), (16, dp([np.inf, 0.013, 0.016])), (17, None), (18, None))
        for i, v in bad_target:
            bad = target()
            bad[i] = v
            assert lib.rsf_law_logtarget(*bad) == -1 and name in lib.rsf_last_error(), i
        assert lib.rsf_law_logtarget(None, *target()[1:]) == -1 and name in lib.rsf_last_error()
        bad = target()  # a logged parameter needs lo > 0
        bad[8], bad[15] = i32([1, 0, 0]), dp([0.0, 0.009, 0.012])
        assert lib.rsf_law_logtarget(*bad) == -1 and name in lib.rsf_last_error()
        pts = target()  # the points: n, z, m and L are not read; npoints >= 1
        pts[4] = pts[5] = pts[6] = pts[7] = None
        pts[10], pts[11] = N, P(th)
        assert lib.rsf_law_logtarget(*pts) == 0
        pts[10] = 0
        assert lib.rsf_law_logtarget(*pts) == -1 and name in lib.rsf_last_error()
        name = b"rsf_law_grid_moments"
        bad_moments = ((1, 2), (2, None), (2, i32([1, 3, 3])), (3, None), (4, None), (4, dp(-w)), (5, None), (5, dp([np.inf, 0.011, 0.014])), (6, None),
                       (6, dp([-0.25, 0.0, 1e-4, 0.0, 0.0, 1e-4])), (7, None), (8, None), (8, i32([1, 1, 2])), (9, None), (10, None), (11, np.nan), (11, np.inf),
                       (12, None), (12, dp([np.nan, 0.0, 0.0])), (14, None))
        for i, v in bad_moments:
            bad = moments()
            bad[i] = v
            assert lib.rsf_law_grid_moments(*bad) == -1 and name in lib.rsf_last_error(), i
        assert lib.rsf_law_grid_moments(None, *moments()[1:]) == -1 and name in lib.rsf_last_error()
        # the integrator: RSF_ERR_UNSUPPORTED
        plain = pkg.RateStateModel(number_time_steps=500)
        plain.integrator = "dop853"
        eng.set_model(plain, 1)
        assert lib.rsf_law_logtarget(*target()) == -5 and b"rsf_law_logtarget" in lib.rsf_last_error()
