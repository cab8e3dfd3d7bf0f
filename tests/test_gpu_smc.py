"""
GPU tests of the tempered sequential Monte Carlo sampler (include/rsf_smc.h: rsf_smc_init / _weight_sums / _resample / _move /
_move_propose / _move_accept / _std2; Engine.smc*, MCMC.sample_smc) against the long double specification tests/smc_reference.py.

Bounds (tests/smc_cases.py, where the measurements and the reasoning are recorded): the start 8 x 2.3e-16 relative, the weight sums
8 x 1.9e-16 relative, the prefix sums 8 x 8.2e-15 relative, the chain step for step 2.4e-10; the fused kernel's l within
shape x 1e-9 of the split path fed with rsf_forward_batch's SSq (tier 1's rtol on SSq through the logarithm); the end-to-end
estimates within Z_MAX = 4.5 standard errors taken from the replicates.
"""
import ctypes

import numpy as np
import pytest

import evidence_cases
import posterior_reference as R
import smc_cases as cases
import smc_reference as ref

pytestmark = pytest.mark.gpu

LD = np.longdouble
_CACHE = {}


def _real_problem(pkg, cpu_engine, dc_true=1000.0):
    """the real model at nsteps 500 and an observation at 1 % noise (tools/evidence_bench.py's recipe) → (model, data)"""
    key = ("real", dc_true)
    if key not in _CACHE:
        model = pkg.RateStateModel(number_time_steps=500)
        model.RadiationDamping = True
        cpu_engine.set_model(model, 1)
        truth = np.asarray(cpu_engine.forward([dc_true])[1])[:, 0]
        _CACHE[key] = truth + 0.01 * np.abs(truth).max() * np.random.default_rng(1).standard_normal(truth.size)
    model = pkg.RateStateModel(number_time_steps=500)
    model.RadiationDamping = True
    return model, _CACHE[key]


# ---- 1. the start ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_init(gpu_engine, d):
    lo, hi = cases.BOXES[d]
    nmax, seed = max(cases.NS), 11
    want = ref.init(seed, cases.OFFSET, nmax, lo, hi, LD)
    for n in cases.NS:
        q = gpu_engine.smc_init(lo, hi, n, seed, cases.OFFSET)
        e = float(np.abs((q - want[:n]) / want[:n]).max())
        print(f"d {d} n {n}: start {e:.3e} (relative)")
        assert q.shape == (n, d) and e <= cases.TOL_INIT and ref.inbox(q, lo, hi).all()
    # shards with offsets form one stream
    k = 300
    a, b = gpu_engine.smc_init(lo, hi, k, seed, cases.OFFSET), gpu_engine.smc_init(lo, hi, nmax - k, seed, cases.OFFSET + k)
    np.testing.assert_array_equal(np.concatenate([a, b]), q)
    # the rule, restated from the probes: u_0 is the uniform of draws, the words are philox's
    for j in (0, 5):
        u0 = gpu_engine.draws(seed, cases.OFFSET + j, 0, d, 12.0)[1]
        assert abs(q[j, 0] - (lo[0] + u0 * (hi[0] - lo[0]))) <= 2 * np.spacing(q[j, 0])
        w = gpu_engine.philox((cases.OFFSET + j, 0, 0, ref.SLOT_U), (seed, 0))
        np.testing.assert_array_equal(ref.words(seed, [cases.OFFSET + j], 0, ref.SLOT_U)[0], w)
    # a box one ulp wide still holds its particles strictly inside ... of two ulp: the only value inside
    lo1 = np.array([1.0])
    hi1 = np.nextafter(np.nextafter(lo1, 2.0), 2.0)
    assert (gpu_engine.smc_init(lo1, hi1, 257, seed) == np.nextafter(lo1, 2.0)).all()


# ---- 2. the weights' sums ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.NS)
def test_weight_sums(pkg, gpu_engine, n):
    l = cases.crafted_l(n)
    got = gpu_engine.smc_weight_sums(l, cases.DELTAS)
    lmax, nfin, nneg, want = ref.weight_sums(l, cases.DELTAS, None, LD)
    assert (got["lmax"], got["n_finite"], got["n_neginf"]) == (lmax, nfin, nneg) and nfin + nneg == n
    e = float(np.abs((got["sums"].astype(LD) - want) / want).max())
    print(f"n {n}: weight sums {e:.3e} (relative, bound {cases.TOL_SUMS:.1e})")
    assert e <= cases.TOL_SUMS
    # two calls, and host and device memory: the same bits
    np.testing.assert_array_equal(gpu_engine.smc_weight_sums(l, cases.DELTAS)["sums"], got["sums"])
    with pkg.Engine(mem="device") as dev:
        np.testing.assert_array_equal(dev.smc_weight_sums(l, cases.DELTAS)["sums"], got["sums"])
    # a given lmax: three uneven shards add to one call
    parts = sum(gpu_engine.smc_weight_sums(l[s], cases.DELTAS, lmax)["sums"] for s in evidence_cases.shards(n) if l[s].size and np.isfinite(l[s]).any())
    if n >= 63:
        np.testing.assert_allclose(parts, got["sums"], rtol=1e-12, atol=0)
    with pytest.raises(pkg.RsfError, match="every particle has l = -inf") as ei:
        gpu_engine.smc_weight_sums(np.full(n, -np.inf), [0.5])
    assert ei.value.code == -1
    bad = l.copy()
    bad[n // 2] = np.nan
    with pytest.raises(pkg.RsfError, match="NaN"):
        gpu_engine.smc_weight_sums(bad, [0.5])


def test_next_delta_follows_the_specification(gpu_engine):
    l = cases.crafted_l(1037)
    got = gpu_engine.smc_next_delta(l, 0.0)
    delta, lmax, sw, ess, beta = ref.choose_delta(0.0, 0.5, lambda cand: ref.weight_sums(l, cand, None, LD))
    assert (got["delta"], got["beta"], got["lmax"]) == (delta, beta, lmax)
    # at a step that is not one of DELTAS the exponents' rounding counts as it does in the prefix sums: TOL_CUM
    assert got["sum_w"] == pytest.approx(float(sw), rel=cases.TOL_CUM) and got["ess"] == pytest.approx(ess, rel=4 * cases.TOL_CUM)
    assert gpu_engine.smc_next_delta(np.zeros(63), 0.25)["beta"] == 1.0


# ---- 3. the scan and the ancestors ----------------------------------------------------------------------------------------------
def _check_resample(eng, q, l, delta, lmax, u):
    n = l.size
    cum, anc, qo, lo_ = eng.smc_resample(q, l, delta, lmax, u)
    want_cum, _ = ref.resample(l, delta, lmax, u, LD)
    nz = want_cum > cases.CUM_FLOOR
    e = float(np.abs((cum[nz].astype(LD) - want_cum[nz]) / want_cum[nz]).max()) if nz.any() else 0.0
    assert e <= cases.TOL_CUM, e
    assert (np.diff(cum) >= 0).all() and (np.diff(anc) >= 0).all() and anc.min() >= 0 and anc.max() < n
    # against the kernel's own cum, exactly: cum[a - 1] <= t_j < cum[a], t_j = ((j + u) W) / n in float64
    t = ((np.arange(n, dtype=np.float64) + u) * cum[-1]) / n
    inside = t < cum[-1]
    below = np.where(anc > 0, cum[np.maximum(anc - 1, 0)], 0.0)
    assert (below[inside] <= t[inside]).all() and (t[inside] < cum[anc][inside]).all()
    assert (cum[anc][~inside] == cum[-1]).all() and (below[~inside] < cum[-1]).all()
    # a particle without weight has no offspring; q and l are gathered through the ancestors
    w = np.where(np.isfinite(l), np.exp(delta * (np.where(np.isfinite(l), l, 0.0) - lmax)), 0.0)
    assert (w[anc] > 0).all()
    np.testing.assert_array_equal(qo, q[anc])
    np.testing.assert_array_equal(lo_, l[anc])
    return e, cum, anc


@pytest.mark.parametrize("n", cases.NS)
def test_scan_and_ancestors(gpu_engine, n):
    rng = np.random.default_rng(n)
    q = rng.uniform(size=(n, 3))
    l = cases.crafted_l(n)
    lmax = float(l[np.isfinite(l)].max())
    worst = max(_check_resample(gpu_engine, q, l, delta, lmax, u)[0] for delta in (1e-4, 0.01, 1.0) for u in (0.37, 1.0, 2.0 ** -53))
    print(f"n {n}: cum {worst:.3e} (relative, bound {cases.TOL_CUM:.1e})")
    # one particle holds all the weight
    one = np.full(n, -np.inf)
    one[n // 3] = -5.0
    _, _, anc = _check_resample(gpu_engine, q, one, 0.5, -5.0, 0.5)
    assert (anc == n // 3).all()
    # prefix sums that are exact in float64: the ancestors are the specification's, one for one
    ex = cases.exact_l(n)
    for u in (0.37, 1.0):
        _, cum, anc = _check_resample(gpu_engine, q[:, :1], ex, 0.25, 0.0, u)
        want_cum, want_anc = ref.resample(ex, 0.25, 0.0, u, LD)
        np.testing.assert_array_equal(cum, np.asarray(want_cum, dtype=np.float64))
        np.testing.assert_array_equal(anc, want_anc)


def test_resample_device_memory_gives_the_same_bits(pkg, gpu_engine):
    n = 16421
    q, l = np.random.default_rng(1).uniform(size=(n, 3)), cases.crafted_l(n)
    lmax = float(l[np.isfinite(l)].max())
    host = gpu_engine.smc_resample(q, l, 0.01, lmax, 0.37)
    with pkg.Engine(mem="device") as dev:
        for a, b in zip(host, dev.smc_resample(q, l, 0.01, lmax, 0.37)):
            np.testing.assert_array_equal(a, b.cpu().numpy())


# ---- 4. the chain logic through the split path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_chain_logic_through_the_split_path(gpu_engine, d):
    _, fn, c = R.closed_reference(d)
    ssq_fn = lambda q: fn(*np.asarray(q).reshape(-1, d).T)
    n, seed = 1037, 3
    got = gpu_engine.smc_from_ssq(ssq_fn, c["lo"], c["hi"], n, c["shape"], seed=seed, history=True)
    want = ref.run(ssq_fn, c["lo"], c["hi"], n, c["shape"], seed=seed, history=True)
    assert [s["beta"] for s in got["stages"]] == [s["beta"] for s in want["stages"]]  # the stage count and every temperature
    width = np.asarray(c["hi"]) - np.asarray(c["lo"])
    differing, eq, el, agree = 0, 0.0, 0.0, np.ones(n, dtype=bool)
    for s, (g, w) in enumerate(zip(got["history"], want["history"])):
        assert g["u"] == w["u"] and g["lmax"] == pytest.approx(w["lmax"], abs=cases.TOL_CHAIN * c["shape"])
        diff = g["ancestors"] != w["ancestors"]
        if diff.any():  # allowed only where t_j lies within 8 ulp of a boundary of cum
            t = ((np.flatnonzero(diff) + g["u"]) * g["cum"][-1]) / n
            near = np.abs(g["cum"][np.minimum(g["ancestors"][diff], w["ancestors"][diff])] - t) <= 8 * np.spacing(t)
            assert near.all()
        differing += int(diff.sum())
        agree = agree[w["ancestors"]] & ~diff  # a lineage that parted once stays apart
        if not agree.all():
            continue  # the populations' covariances differ from here on: nothing tighter than the counts holds
        for (gq, gl), (wq, wl) in zip(g["after"], w["after"]):
            eq, el = max(eq, float((np.abs(gq - wq) / width).max())), max(el, float(np.abs(gl - wl).max()))
        assert got["stages"][s]["accept_rate"] == want["stages"][s]["accept_rate"]
    print(f"d {d}: {len(got['stages'])} stages, {differing} differing ancestors, q {eq:.3e} (of the box), l {el:.3e}")
    assert differing <= 1e-3 * n
    assert eq <= cases.TOL_CHAIN and el <= cases.TOL_CHAIN * c["shape"]
    assert got["log_integral"] == pytest.approx(want["log_integral"], abs=1e-9)
    assert got["log_evidence"] == pytest.approx(ref.log_evidence(got["log_integral"], c["shape"], c["lo"], c["hi"]), abs=1e-12)
    assert np.isfinite(got["std2"]).all() and (got["std2"] > 0).all()


# ---- 5. the fused kernel against the split path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("d", [1, 3])
def test_fused_against_split(pkg, gpu_engine, cpu_engine, d, damping):
    model, data = _real_problem(pkg, cpu_engine)
    model.RadiationDamping = damping
    gpu_engine.set_model(model, 1)
    n, seed, beta, it = 1037, 5, 0.37, 4
    lo, hi = np.array([600.0, 0.009, 0.013])[:d], np.array([1600.0, 0.013, 0.017])[:d]
    shape = 0.5 * data.size
    rng = np.random.default_rng(d)
    q = np.ascontiguousarray(np.column_stack([rng.uniform(600.0, 1600.0, n), rng.uniform(0.009, 0.013, n), rng.uniform(0.013, 0.017, n)])[:, :d])
    q[:64, 0] = np.linspace(1599.0, 1599.9, 64)  # a wave next to the edge: with the wide factor below most of it proposes outside
    chol = np.diag([120.0, 4e-4, 4e-4][:d]) + (np.array([[0, 0, 0], [-1e-4, 0, 0], [1e-5, -2e-5, 0]])[:d, :d])
    ssq = lambda x: np.asarray(gpu_engine.forward(x[:, 0], a=x[:, 1] if d == 3 else None, b=x[:, 2] if d == 3 else None, data=data,
                                                  want_ssq=True, want_acc=False)[0])
    l = -shape * np.log(ssq(q))
    qn, inb = gpu_engine.smc_move_propose(q, lo, hi, chol, seed, cases.OFFSET, it)
    inb = inb.astype(bool)
    sn = np.ones(n)
    sn[inb] = ssq(qn[inb])
    q_split, l_split, acc_split = gpu_engine.smc_move_accept(q, l, qn, inb, sn, shape, beta, seed, cases.OFFSET, it)
    q_fused, l_fused, acc_fused = gpu_engine.smc_move(q, l, data, lo, hi, chol, beta, seed, cases.OFFSET, it, 1)
    assert 0 < inb.sum() < n and 0 < acc_split < inb.sum()
    # decisions are identical except proven near-ties: |beta (l' - l) - log u| within the bound on l'
    moved_s, moved_f = (q_split != q).any(axis=1), (q_fused != q).any(axis=1)
    fork = moved_s != moved_f
    if fork.any():
        logu = np.log(ref.accept_uniforms(seed, cases.OFFSET + np.flatnonzero(fork).astype(np.uint64), it))
        margin = np.abs(beta * (-shape * np.log(sn[fork]) - l[fork]) - logu)
        assert (margin <= beta * shape * 1e-9).all(), margin
    same = ~fork
    np.testing.assert_array_equal(q_fused[same], q_split[same])
    e = float(np.abs(l_fused[same] - l_split[same]).max())
    print(f"d {d} damping {damping}: {int(inb.sum())} inside the box, {acc_split} accepted, {int(fork.sum())} near-ties, l within {e:.3e} "
          f"(bound {shape * 1e-9:.3e})")
    assert e <= shape * 1e-9 and int(acc_fused[0]) == int(moved_f.sum())
    # three steps in one launch are three launches of one step
    qa, la, acc3 = gpu_engine.smc_move(q, l, data, lo, hi, chol, beta, seed, cases.OFFSET, it, 3)
    qb, lb, accs = q, l, []
    for k in range(3):
        qb, lb, a = gpu_engine.smc_move(qb, lb, data, lo, hi, chol, beta, seed, cases.OFFSET, it + k, 1)
        accs.append(int(a[0]))
    np.testing.assert_array_equal(qa, qb)
    np.testing.assert_array_equal(la, lb)
    assert [int(a) for a in acc3] == accs


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------
def test_end_to_end_real_model(pkg, gpu_engine, cpu_engine):
    model, data = _real_problem(pkg, cpu_engine)
    cpu_engine.set_model(model, 1)
    gpu_engine.set_model(model, 1)
    shape, lo, hi = 0.5 * data.size, 0.0, 1.0e4
    fn = R.checker_ssq(cpu_engine, data)
    post = R.Posterior1(fn, lo, hi, shape, n_fine=4001)
    truth = np.log(post.Z) + post.lmax
    runs = [gpu_engine.smc(data, [lo], [hi], cases.N_SPEC, seed=s) for s in range(8)]
    logi = np.array([r["log_integral"] for r in runs])
    ratio = np.exp(logi - truth)
    z = (ratio.mean() - 1.0) / (ratio.std(ddof=1) / np.sqrt(ratio.size))
    print(f"real model d = 1: truth {truth:.5f}, log I {logi.mean():.5f} +- {logi.std(ddof=1):.4f} over 8 seeds (specification's sd "
          f"{cases.SPEC_SD_REAL}), ratio z {z:+.2f}, {len(runs[0]['stages'])} stages, accept rates "
          f"{[round(s['accept_rate'], 3) for s in runs[0]['stages']]}")
    assert abs(z) < R.Z_MAX
    assert logi.std(ddof=1) <= cases.SD_RATIO_MAX * cases.SPEC_SD_REAL
    fails = []
    R.check("smc real d=1", post, runs[0]["q"], runs[0]["std2"], fails)
    assert not fails, fails
    assert runs[0]["stages"][-1]["beta"] == 1.0 and runs[0]["n_solves"] == cases.N_SPEC * (1 + 3 * len(runs[0]["stages"]))


def test_end_to_end_closed_form_d3(gpu_engine):
    _, fn, c = R.closed_reference(3)
    ssq_fn = lambda q: fn(*np.asarray(q).reshape(-1, 3).T)
    logi = np.array([gpu_engine.smc_from_ssq(ssq_fn, c["lo"], c["hi"], cases.N_SPEC, c["shape"], seed=100 + s)["log_integral"] for s in range(8)])
    ratio = np.exp(logi - evidence_cases.CLOSED_TRUTH[3])
    z = (ratio.mean() - 1.0) / (ratio.std(ddof=1) / np.sqrt(ratio.size))
    print(f"closed form d = 3: log I {logi.mean():.5f} +- {logi.std(ddof=1):.4f} (truth {evidence_cases.CLOSED_TRUTH[3]}), ratio z {z:+.2f}")
    assert abs(z) < R.Z_MAX and logi.std(ddof=1) <= cases.SD_RATIO_MAX * cases.SPEC_SD[3]


def test_the_bad_start_goes_away(pkg, gpu_engine, cpu_engine):
    """main.py's Dc_true = 100 group with the prior box of its sweep, (0, 1e4): the random walk started at 1000 spends its proposals
    outside the box and accepts 1 %; the particles start uniform in the box and reach the posterior."""
    model, data = _real_problem(pkg, cpu_engine, dc_true=100.0)
    cpu_engine.set_model(model, 1)
    gpu_engine.set_model(model, 1)
    shape = 0.5 * data.size
    post = R.Posterior1(R.checker_ssq(cpu_engine, data), 0.0, 1.0e4, shape, n_fine=4001)
    runs = [gpu_engine.smc(data, [0.0], [1.0e4], 4096, seed=s) for s in range(8)]
    res = runs[0]
    print(f"Dc_true = 100: {len(res['stages'])} stages, accept rates {[round(s['accept_rate'], 3) for s in res['stages']]}")
    # The particles of one run share ancestors, so they are not the independent states posterior_reference.check assumes (a stage
    # that accepts little leaves copies): the standard errors come from the replicates, as in tests/test_smc_reference.py
    mg = post.marg["Dc"]
    m, v = np.array([r["q"].mean() for r in runs]), np.array([r["q"].var() for r in runs])
    zm = (m.mean() - mg.mean) / (m.std(ddof=1) / np.sqrt(m.size))
    zv = (v.mean() - mg.var) / (v.std(ddof=1) / np.sqrt(v.size))
    print(f"Dc_true = 100: mean Dc {m.mean():.4f} (exact {mg.mean:.4f}, z {zm:+.2f}), variance {v.mean():.5f} (exact {mg.var:.5f}, z {zv:+.2f})")
    assert abs(zm) < R.Z_MAX and abs(zv) < R.Z_MAX
    assert all(r["stages"][-1]["beta"] == 1.0 and ref.inbox(r["q"], [0.0], [1.0e4]).all() for r in runs)
    # every particle is within the posterior's reach of the truth: none is left where it started
    assert all((np.abs(r["q"] - mg.mean) < R.WINDOW_SD * mg.sd).all() for r in runs)


def test_the_pool_is_a_pool(pkg, cpu_engine):
    model, data = _real_problem(pkg, cpu_engine)
    m = pkg.MCMC(model, data, 1000.0, ["Uniform", 0.0, 1.0e4], 1000.0, nsamples=10, verbose=False)
    pool = m.sample_smc(4096, seed=2)
    assert isinstance(pool, pkg.PosteriorPool) and pool.samples.shape == (16, 256, 1) and pool.std2.shape == (16, 256)
    assert pool.stats["stages"][-1]["beta"] == 1.0 and 0.0 < pool.accept_rate < 1.0
    pred = pool.loo(model, data, max_draws=1024)
    assert np.isfinite(pred["elpd_loo"]) and np.isfinite(pred["elpd_waic"]) and pred["mean"].shape == data.shape
    j = pool.joint()
    assert j["n"] == 4096 and j["nonfinite"] == 0 and j["cov"].shape == (1, 1)
    ev = pool.evidence(model, data, [0.0], [1.0e4])
    se = np.hypot(ev["re"], cases.SPEC_SD_REAL)
    print(f"log p(y | M): bridge {ev['log_evidence']:.4f} (re {ev['re']:.2e}), SMC {pool.stats['log_evidence']:.4f} (sd {cases.SPEC_SD_REAL})")
    assert ev["converged"] and abs(ev["log_evidence"] - pool.stats["log_evidence"]) < R.Z_MAX * se


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, gpu_engine):
    E = pkg.RsfError

    def code(fn, *a, **kw):
        with pytest.raises(E) as ei:
            fn(*a, **kw)
        return ei.value.code, str(ei.value)

    assert code(gpu_engine.smc_init, [0.0], [1.0], 0)[0] == -1
    assert code(gpu_engine.smc_init, [1.0], [1.0], 10)[0] == -1
    assert code(gpu_engine.smc_init, [0.0], [1.0], 10, offset=-1)[0] == -1
    assert code(gpu_engine.smc_init, [0.0] * 4, [1.0] * 4, 10)[0] == -1
    q, l = np.full((4, 1), 1000.0), np.zeros(4)
    with pytest.raises(E, match="set_model"):
        gpu_engine.smc_move(q, l, np.zeros(500), [0.0], [1e4], [[1.0]], 0.5)
    lib, dbl = gpu_engine.lib, ctypes.POINTER(ctypes.c_double)
    one, acc = np.ones(4), np.zeros(4, dtype=np.int64)
    P = lambda x: x.ctypes.data_as(dbl)
    assert lib.rsf_smc_move(gpu_engine._ctx, 4, 1, q.ctypes.data, l.ctypes.data, one.ctypes.data, 12.0, P(one * 0), P(one), P(one), 0.5, 0, 0, 1, 1,
                            acc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == -3  # no model: RSF_ERR_STATE
    model = pkg.RateStateModel(number_time_steps=50)
    gpu_engine.set_model(model, 1)
    data = np.zeros(gpu_engine.nout)
    ok = (q, l, data, [0.0], [1e4], [[1.0]], 0.5)
    assert gpu_engine.smc_move(*ok)[0].shape == (4, 1)
    assert code(gpu_engine.smc_move, np.ones((4, 2)), l, data, [0.0, 0.0], [1.0, 1.0], np.eye(2), 0.5) == (-1, "rsf error -1: rsf_smc_move: need d = 1 or 3")
    assert code(gpu_engine.smc_move, np.ones((0, 1)), np.zeros(0), *ok[2:])[0] == -1  # n = 0
    assert "lo[0] < hi[0]" in code(gpu_engine.smc_move, q, l, data, [1e4], [0.0], [[1.0]], 0.5)[1]
    assert "shape" in code(gpu_engine.smc_move, *ok, shape=0.0)[1] and code(gpu_engine.smc_move, *ok, shape=-1.0)[0] == -1
    assert code(gpu_engine.smc_move, *ok[:5], [[0.0]], 0.5)[0] == -1 and code(gpu_engine.smc_move, *ok[:6], 0.0)[0] == -1
    assert code(gpu_engine.smc_move, *ok, steps=0)[0] == -1 and code(gpu_engine.smc_move, *ok, iter0=0)[0] == -1
    assert code(gpu_engine.smc_resample, q, l, 0.5, 0.0, 0.0)[0] == -1 and code(gpu_engine.smc_resample, q, l, -0.5, 0.0, 0.5)[0] == -1
    assert code(gpu_engine.smc_std2, l, 0.5)[0] == -1
    with pytest.raises(ValueError):
        gpu_engine.smc(data, [0.0, 0.0], [1.0, 1.0], 10)  # d = 2
    with pytest.raises(ValueError):
        gpu_engine.smc(data, [0.0], [1.0], 10, ess_fraction=1.0)
    assert code(gpu_engine.smc, data, [0.0], [1.0], 0)[0] == -1
    assert code(gpu_engine.smc, data, [1.0], [0.0], 10)[0] == -1
    assert code(gpu_engine.smc, data, [0.0], [1e4], 10, shape=-2.0)[0] == -1
    model.integrator = "dop853"
    gpu_engine.set_model(model, 1)
    assert code(gpu_engine.smc_move, *ok)[0] == -5 and "DOP853" in code(gpu_engine.smc, data, [0.0], [1e4], 10)[1]
