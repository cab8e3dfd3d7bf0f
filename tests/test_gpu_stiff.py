"""
GPU tests of the state-law solve and its delayed-rejection sampler with the stiffness of the apparatus a model constant,
independent of Dc (include/rsf_stiff.h: rsf_stiff_observe / rsf_stiff_dr_run / rsf_stiff_dr_ssq; Engine.stiff_*, the stiffness
keyword of the law_* calls, RateStateModel.stiffness, MCMC):
  4. the coupling identity: where k Dc == 0.1 exactly the new kernels are rsf_law_observe / rsf_law_dr_ssq bit for bit;
  5. accuracy against the long-double specification (tests/stiff_reference.py) at k = 4e-3;
  6. lanes whose trajectory is not finite at k = 1e-3, in the solve and in the sampler;
  7. the fused kernel against the split path rsf_dr_propose -> rsf_stiff_observe -> rsf_dr_accept, bit for bit;
  8. the target: MCMC.sample_law keeps the quadrature's posterior on constant-stiffness data, which the coupled model cannot fit;
  9. the front end, and stiffness=None is the parent's path.
Shapes: nsteps 500 unless the matrix entry says otherwise; 12 lanes, and 70 (the twelve tiled: a full wave and a partial one).
"""
import functools

import numpy as np
import pytest

import law_cases as C
import law_dr_reference as LS
import law_matrix_cases as M
import law_reference as R
import observe_reference as O
import stiff_cases as SC
import stiff_reference as S

pytestmark = pytest.mark.gpu

COUNTERS = ("accepted1", "accepted2", "outbox1", "outbox2", "stuck")
GAMMA, SEED, OFFSET = 0.3, 5, 900
BOX = {1: (np.array([R.BF_BOX[0]]), np.array([R.BF_BOX[1]])), 3: (LS.LO3, LS.HI3)}
SENT = -7.25


def _model(pkg, m, table, **attrs):
    """the package's model of the specification's attributes `m`, its loading `table`"""
    model = pkg.RateStateModel(number_time_steps=m.num_tsteps, start_time=m.t_start, end_time=m.t_final)
    for k in ("a", "b", "mu_ref", "V_ref", "k1", "mu_t_zero", "RadiationDamping", "substeps"):
        setattr(model, k, getattr(m, k))
    model.loading = table
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def _bits(x):
    x = np.ascontiguousarray(np.asarray(x.cpu() if hasattr(x, "cpu") else x))
    return x.view(np.int32 if x.dtype.itemsize == 4 else (np.uint8 if x.dtype.itemsize == 1 else np.int64))


def _tile(x, idx):
    return None if x is None else np.ascontiguousarray(np.asarray(x)[idx])


def _noisy(clean, seed):
    return clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(seed).standard_normal(clean.size)


# ---- 4. the coupling identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k1", [None, 0.0], ids=["damped", "k1zero"])
@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("law", R.LAWS)
def test_coupling_identity(pkg, gpu_engine, law, history, k1):
    """Lanes at Dc = 64 with per-lane (a, b) and k = 0.1 / 64: kappa = k Dc is 0.1 and ikappa its reciprocal exactly, every lane
    constant is the coupled kernel's, and rsf_stiff_observe returns rsf_law_observe's series and SSq bit for bit — all four
    observables, 12 lanes and 70."""
    m = C.spec() if k1 is None else C.spec(k1=k1)
    eng = gpu_engine
    eng.set_model(_model(pkg, m, R.table(m, history)), 1)
    assert eng.stiffness is None
    dc12, a12, b12 = SC.coupled_lanes()
    for idx in (np.arange(12), SC.lanes70()):
        dc, a, b = dc12[idx], a12[idx], b12[idx]
        for obs in O.OBSERVABLES:
            want = eng.law_observe(law, obs, dc, a, b)[1]
            data = _noisy(np.asarray(want)[:, 3], 4)
            want_ssq = eng.law_observe(law, obs, dc, a, b, data=data, want_ssq=True, want_series=False)[0]
            ssq, got = eng.stiff_observe(law, obs, SC.K64, dc, a, b, data=data, want_ssq=True, want_series=True)
            assert np.isfinite(want).all() and np.isfinite(want_ssq).all() and np.abs(np.asarray(want) - np.asarray(want)[0]).max() > 0, obs
            assert np.array_equal(_bits(got), _bits(want)), (obs, idx.size)
            assert np.array_equal(_bits(ssq), _bits(want_ssq)), (obs, idx.size)
            # ... and it is the stiffness that does it: twice as stiff is another series
            assert not np.array_equal(np.asarray(eng.stiff_observe(law, obs, 2.0 * SC.K64, dc, a, b)[1])[1:], np.asarray(want)[1:]), obs


# ---- 5. accuracy -------------------------------------------------------------------------------------------------------------------------
def _gate(tag, obs, got, s, idx, lanes=None):
    """print one series' error against long double and return it with the entry's yardstick; lanes: the specification's lanes held
    to the bound (default: all)"""
    got = np.asarray(got)
    ext = s["ext"][obs][:, idx]
    keep = np.ones(idx.size, dtype=bool) if lanes is None else lanes[idx]
    assert got.shape == ext.shape and np.isfinite(got[:, keep]).all(), (tag, obs)
    err, yard = M.error(obs, got[:, keep], ext[:, keep]), s["yardstick"][obs]
    print(f"{tag} {obs} ({idx.size} lanes): GPU {err.max():.2e}, yardstick {yard:.2e} (own {s['own'][obs]:.2e}), ratio {err.max() / yard:.2f}")
    return obs, float(err.max()), yard


def _assert_gates(tag, gates):
    for obs, err, yard in gates:
        assert err < C.CAP, (tag, obs)
        assert err <= 4.0 * yard, (tag, obs)


@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("name", SC.ENTRIES)
def test_against_long_double(pkg, gpu_engine, name, law, history):
    """k = 4e-3: per entry and observable the GPU's largest error against the long-double specification — law_matrix_cases.error's
    measure — is below law_cases.CAP and at most 4 x the entry's yardstick (the larger of the two CPU arrangements' largest error,
    floored at the default model's: tests/test_gpu_law_matrix.py's bound), on every lane, 12 lanes and 70."""
    s = SC.solve(name, history, law)
    eng = gpu_engine
    eng.set_model(_model(pkg, s["m"], s["vl"], stiffness=SC.K_ACC), s["m"].substeps)
    assert eng.nout == R.nout(s["m"]) and eng.stiffness == SC.K_ACC and s["finite"].all()
    tag = f"{name} {history} {law}"
    gates, first = [], {}
    for idx in (np.arange(12), SC.lanes70()):
        dc, a, b = s["dc"][idx], _tile(s["a"], idx), _tile(s["b"], idx)
        for obs in O.OBSERVABLES:
            got = np.asarray(eng.law_observe(law, obs, dc, a, b)[1])  # the engine's model's stiffness: rsf_stiff_observe
            gates.append(_gate(tag, obs, got, s, idx))
            if idx.size == 12:
                first[obs] = got
                assert np.array_equal(_bits(got), _bits(eng.stiff_observe(law, obs, SC.K_ACC, dc, a, b)[1])), obs
            else:  # a lane's series does not depend on its neighbours
                assert np.array_equal(_bits(got), _bits(first[obs][:, idx])), obs
    _assert_gates(tag, gates)


# ---- 6. lanes that are not finite ----------------------------------------------------------------------------------------------------------
def test_non_finite_lanes(pkg, gpu_engine):
    """k = 1e-3 under the step history and the slip law: the specification is non-finite on exactly the lanes Dc = 5, 6, 8.  There
    the GPU's SSq is non-finite; on the other nine the series meet test 5's bound.  A chain started on such a lane is refused as a
    start; a chain that proposes such a point stays where it is, and no chain ever sits on one."""
    law, obs = "slip", "mu"
    s = SC.solve("default", "step", law, SC.K_LOW)
    bad = np.isin(s["dc"], SC.LOW_LANES)
    assert np.array_equal(s["finite"], ~bad)
    eng = gpu_engine
    eng.set_model(_model(pkg, s["m"], s["vl"], stiffness=SC.K_LOW, state_law=law, observable=obs), 1)
    data = _noisy(s["spec"][obs][:, R.LANES.index(R.BF_TRUTH)], 4)
    gates = []
    for idx in (np.arange(12), SC.lanes70()):
        ssq = np.asarray(eng.law_observe(law, obs, s["dc"][idx], data=data, want_ssq=True, want_series=False)[0])
        assert np.array_equal(np.isfinite(ssq), ~bad[idx]), ssq
        ext = ((s["ext"][obs][:, idx] - data.astype(R.LD)[:, None]) ** 2).sum(axis=0).astype(np.float64)
        assert (np.abs(ssq[~bad[idx]] - ext[~bad[idx]]) <= 1e-9 * ext[~bad[idx]]).all()
        for o in O.OBSERVABLES:
            gates.append(_gate("k 1e-3 step slip", o, eng.law_observe(law, o, s["dc"][idx])[1], s, idx, lanes=~bad))
    _assert_gates("k 1e-3 step slip", gates)
    # the sampler: a start on such a lane is refused, as law_dr refuses any start without a finite l
    lo, hi = BOX[1]
    n = 128
    q0 = np.full((n, 1), 10.0)
    q0[5, 0] = 6.0
    with pytest.raises(ValueError, match="stuck start: 1 walkers"):
        eng.law_dr(law, obs, q0, data, lo, hi, [[3.0]], 4)
    # chains at Dc = 10 with a factor of 3: many first proposals land below, where the trajectory is not finite
    q0[:] = 10.0
    shape = 0.5 * eng.nout
    l0 = -shape * np.log(eng.law_ssq_fn(law, data, obs)(q0))
    assert np.isfinite(l0).all()
    kw = dict(gamma=GAMMA, seed=SEED, offset=OFFSET)
    y, mask = eng.dr_propose(q0, l0, lo, hi, [[3.0]], 1, iteration=1, **kw)
    s1 = np.asarray(eng.law_dr_ssq(law, obs, y, mask, data))
    nonfinite = (np.asarray(mask) == 1) & ~np.isfinite(s1)
    print(f"{int(nonfinite.sum())} of {n} first proposals inside the box are not finite")
    assert nonfinite.sum() >= 8
    q, l, cnt = q0.copy(), l0.copy(), [np.zeros(n, dtype=np.int32) for _ in COUNTERS]
    eng.law_dr_run(law, obs, q, l, data, lo, hi, [[3.0]], 1, cnt, stages=1, shape=shape, iter0=1, **kw)
    assert (q[nonfinite, 0] == 10.0).all() and np.array_equal(_bits(l[nonfinite]), _bits(l0[nonfinite])) and (cnt[0][nonfinite] == 0).all()
    assert cnt[0].sum() > 0 and cnt[2][nonfinite].sum() == 0  # others moved; a non-finite point is no out-of-box proposal
    res = eng.law_dr(law, obs, q0, data, lo, hi, [[3.0]], 8, iters_per_launch=4, **kw)
    final = np.asarray(eng.law_ssq_fn(law, data, obs)(np.asarray(res.trace_q).reshape(-1, 1)))
    assert np.isfinite(final).all() and np.isfinite(np.asarray(res.trace_l)).all()


# ---- 7. fused = split ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dr_data(law, obs):
    """two observation series of the constant-k model at the truth (20, 0.011, 0.014), k = 4e-3, step history: two noise draws"""
    m = C.spec()
    clean = S.forward(m, SC.K_ACC, [R.BF_TRUTH], R.table(m, "step"), law, obs)[0][:, 0]
    return np.stack([_noisy(clean, R.BF_SEED), _noisy(clean, R.BF_SEED + 1)])


def _starts(d, n):
    rng = np.random.default_rng(7)
    q = np.column_stack([rng.uniform(15.0, 25.0, n), rng.uniform(0.0105, 0.0115, n), rng.uniform(0.0135, 0.0145, n)])[:, :d]
    return np.ascontiguousarray(q)


def _observe_ssq(eng, law, obs, k, y, mask, data):
    """rsf_stiff_observe's SSq of the masked-in proposals, group by group against the group's series -> (n,), 1 elsewhere"""
    y, mask = np.asarray(y), np.asarray(mask)
    G = data.shape[0]
    per, out = y.shape[0] // G, np.ones(y.shape[0])
    for g in range(G):
        rows = np.flatnonzero(mask[g * per:(g + 1) * per]) + g * per
        if rows.size:
            ab = [np.ascontiguousarray(y[rows, p]) for p in (1, 2)] if y.shape[1] == 3 else [None, None]
            out[rows] = eng.stiff_observe(law, obs, k, np.ascontiguousarray(y[rows, 0]), ab[0], ab[1], data=data[g], want_ssq=True, want_series=False)[0]
    return out


@pytest.mark.parametrize("obs", ["mu", "acc"])
@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("d", [1, 3])
def test_fused_against_split(pkg, d, law, obs):
    """rsf_stiff_dr_run against rsf_dr_propose -> rsf_stiff_observe -> rsf_dr_accept: the state after every iteration and all five
    counters, bit for bit; one and two stages, two observation groups, 128 chains x 8 iterations in two launches of four."""
    n, G, k = 128, 2, SC.K_ACC
    m = C.spec()
    data = _dr_data(law, obs)
    lo, hi = BOX[d]
    shape = 0.5 * data.shape[-1]
    q0 = _starts(d, n)
    per = n // G
    with pkg.Engine(mem="host", block_threads=64) as eng:
        eng.set_model(_model(pkg, m, R.table(m, "step")), 1)  # no stiffness of the model's: every call names it
        L1 = eng.law_gn_factor(law, obs, LS.TRUTH3[:d], data[0], stiffness=k)[0]
        L = np.stack([L1, 2.0 * L1])
        l0 = np.concatenate([-shape * np.log(eng.law_ssq_fn(law, data[g], obs, stiffness=k)(q0[g * per:(g + 1) * per])) for g in range(G)])
        assert np.isfinite(l0).all()
        for stages in (1, 2):
            fused, split = [dict(q=q0.copy(), l=l0.copy(), c=[np.zeros(n, dtype=np.int32) for _ in COUNTERS]) for _ in range(2)]
            for first in (1, 5):
                tq, tl = eng.stiff_dr_run(law, obs, k, fused["q"], fused["l"], data, lo, hi, L, 4, fused["c"], gamma=GAMMA, stages=stages, shape=shape,
                                          seed=SEED, offset=OFFSET, iter0=first, trace=True)
                for j, it in enumerate(range(first, first + 4)):
                    kw = dict(gamma=GAMMA, seed=SEED, offset=OFFSET, iteration=it)
                    y, mk = eng.dr_propose(split["q"], split["l"], lo, hi, L, 1, **kw)
                    l1, pend = eng.dr_accept(split["q"], split["l"], lo, hi, 1, y, mk, _observe_ssq(eng, law, obs, k, y, mk, data), split["c"], shape, **kw)
                    if stages == 2:
                        y, mk = eng.dr_propose(split["q"], split["l"], lo, hi, L, 2, pending=pend, **kw)
                        eng.dr_accept(split["q"], split["l"], lo, hi, 2, y, mk, _observe_ssq(eng, law, obs, k, y, mk, data), split["c"], shape, l1=l1,
                                      pending=pend, **kw)
                    assert np.asarray(tq)[j].tobytes() == split["q"].tobytes() and np.asarray(tl)[j].tobytes() == split["l"].tobytes(), (stages, it)
                same = {key: bool(np.array_equal(_bits(fused[key]), _bits(split[key]))) for key in ("q", "l")}
                same.update({key: bool(np.array_equal(a, b)) for key, a, b in zip(COUNTERS, fused["c"], split["c"])})
                print(f"d {d} {law} {obs} stages {stages} after iteration {first + 3}: counters "
                      f"{ {key: int(v.sum()) for key, v in zip(COUNTERS, fused['c'])} } of {(first + 3) * n}; bit-identical {same}")
                assert all(same.values()), same
            a1, a2, o1, o2, stuck = fused["c"]
            assert a1.sum() > 0 and (a2.sum() > 0) == (stages == 2) and stuck.sum() == 0 and (a1 + a2 <= 8).all()
        # the engine's model's stiffness is what the law_* calls run without the keyword
        eng.set_model(_model(pkg, m, R.table(m, "step"), stiffness=k), 1)
        again = dict(q=q0.copy(), l=l0.copy(), c=[np.zeros(n, dtype=np.int32) for _ in COUNTERS])
        for first in (1, 5):
            eng.law_dr_run(law, obs, again["q"], again["l"], data, lo, hi, L, 4, again["c"], gamma=GAMMA, stages=2, shape=shape, seed=SEED, offset=OFFSET,
                           iter0=first)
        assert np.array_equal(_bits(again["q"]), _bits(fused["q"])) and np.array_equal(_bits(again["l"]), _bits(fused["l"]))


@pytest.mark.parametrize("d", [1, 3])
def test_stage_ssq_is_stiff_observe_bit_for_bit(pkg, d):
    """rsf_stiff_dr_ssq on a mask with an empty wave (lanes 64 .. 127 of 133) against rsf_stiff_observe on the compacted points;
    and at Dc = 64 with k = 0.1 / 64, the proposals varying in (a, b), it is rsf_law_dr_ssq's SSq too."""
    m = C.spec()
    n = 133
    with pkg.Engine(mem="host") as eng:
        eng.set_model(_model(pkg, m, R.table(m, "step")), 1)
        for law in R.LAWS:
            for obs in ("mu", "acc"):
                data = _dr_data(law, obs)[0]
                lo, hi = BOX[d]
                y = np.ascontiguousarray(lo + (hi - lo) * np.random.default_rng([n, d]).uniform(0.05, 0.95, (n, d)))
                mask = ((np.arange(n) % 3 != 2) & ~((np.arange(n) >= 64) & (np.arange(n) < 128))).astype(np.uint8)
                got = np.asarray(eng.stiff_dr_ssq(law, obs, SC.K_ACC, y, mask, data, ssq=np.full(n, SENT)))
                want = _observe_ssq(eng, law, obs, SC.K_ACC, y, mask, data[None])
                rows = mask == 1
                assert np.isfinite(want[rows]).all() and np.array_equal(_bits(got[rows]), _bits(want[rows])), (law, obs)
                assert (got[~rows] == SENT).all(), (law, obs)
                if d == 3:
                    y64 = y.copy()
                    y64[:, 0] = SC.DC64
                    ones = np.ones(n, dtype=np.uint8)
                    coupled = np.asarray(eng.law_dr_ssq(law, obs, y64, ones, data))
                    stiff = np.asarray(eng.stiff_dr_ssq(law, obs, SC.K64, y64, ones, data))
                    assert np.isfinite(coupled).all() and np.unique(coupled).size > n // 2
                    assert np.array_equal(_bits(stiff), _bits(coupled)), (law, obs)


# ---- 8. the target -----------------------------------------------------------------------------------------------------------------------------
def test_sample_law_keeps_the_quadrature_posterior(pkg):
    """Friction data of the constant-k model (Dc = 20, k = 2e-3, the hold history): MCMC.sample_law at 256 chains x 400 iterations
    against MCMC.quadrature() on the same model by tests/test_gpu_law_dr.py's rule — the mean of the per-chain means within 4.5
    standard errors of the quadrature's mean; the posterior mean lies nearer 20 than 30; and the coupled model's best SSq over
    BF_BOX is at least 3 x the constant-k model's (4.6 x on the CPU specification)."""
    p = SC.why_problem("hold")
    model = _model(pkg, p["m"], p["vl"], observable="mu", stiffness=SC.K_WHY)
    mc = pkg.MCMC(model, p["data"], R.BF_TRUTH, ["Uniform", *R.BF_BOX], R.BF_TRUTH, nsamples=10, verbose=False)
    grid = mc.quadrature()
    try:
        exact = float(np.asarray(grid.mean).reshape(-1)[0])
    finally:
        grid.engine.close()
    pool = mc.sample_law(256, 400, seed=9)
    x = np.asarray(pool.samples)[:, :, 0]
    assert x.shape == (200, 256) and pool.stats["stuck"] == 0 and pool.stats["path"] == "law_dr"
    means = x.mean(axis=0)
    se = means.std(ddof=1) / np.sqrt(means.size)
    z = (means.mean() - exact) / se
    print(f"pooled mean {means.mean():.4f}, quadrature {exact:.4f}, pooled SD {x.std():.4f}, SE {se:.2e}, z {z:+.2f}; accept rate {pool.accept_rate:.2f}")
    assert 0.05 < pool.accept_rate < 0.95
    assert abs(z) < 4.5
    assert abs(means.mean() - 20.0) < abs(means.mean() - 30.0) and abs(exact - 20.0) < abs(exact - 30.0)
    with pkg.Engine(mem="host") as eng:
        eng.set_model(_model(pkg, p["m"], p["vl"], observable="mu"), 1)
        coupled = np.asarray(eng.law_observe("aging", "mu", p["x"], data=p["data"], want_ssq=True, want_series=False)[0])
        stiff = np.asarray(eng.stiff_observe("aging", "mu", SC.K_WHY, p["x"], data=p["data"], want_ssq=True, want_series=False)[0])
    ratio = coupled.min() / stiff.min()
    print(f"best SSq: coupled {coupled.min():.3e} at Dc {p['x'][coupled.argmin()]:.2f}, constant k {stiff.min():.3e} at Dc {p['x'][stiff.argmin()]:.2f}: "
          f"{ratio:.2f} x (CPU {p['ssq_coupled'].min() / p['ssq_stiff'].min():.2f} x); against the CPU specification's SSq "
          f"{np.abs(stiff / p['ssq_stiff'] - 1).max():.2e} and {np.abs(coupled / p['ssq_coupled'] - 1).max():.2e}")
    assert ratio >= 3.0
    assert (np.abs(stiff - p["ssq_stiff"]) <= 1e-9 * p["ssq_stiff"]).all() and (np.abs(coupled - p["ssq_coupled"]) <= 1e-9 * p["ssq_coupled"]).all()


# ---- 9. the front end ----------------------------------------------------------------------------------------------------------------------------
def test_drop_in(pkg, gpu_engine):
    """RateStateModel(stiffness=k).evaluate() and trajectory() return test 5's series (Engine.law_observe's on the same model, bit
    for bit, every observable, "acc" included, under either law); with stiffness=None the result is the parent's path's."""
    s = SC.solve("ab", "step", "slip")
    model = _model(pkg, s["m"], s["vl"], stiffness=SC.K_ACC, state_law="slip")
    eng = gpu_engine
    eng.set_model(model, 1)
    try:
        out = model.trajectory(s["dc"], s["a"], s["b"])
        for obs in O.OBSERVABLES:
            want = np.asarray(eng.stiff_observe("slip", obs, SC.K_ACC, s["dc"], s["a"], s["b"])[1])
            assert np.array_equal(_bits(out[obs]), _bits(want.T)), obs
            assert M.error(obs, out[obs].T, s["ext"][obs]).max() <= 4.0 * s["yardstick"][obs], obs
            model.observable = obs
            assert np.array_equal(_bits(model.evaluate_batch(s["dc"], s["a"], s["b"])), _bits(want.T)), obs
            model.Dc = 20.0
            t, series, noisy = model.evaluate()
            one = np.asarray(eng.stiff_observe("slip", obs, SC.K_ACC, [20.0])[1])[:, 0]
            assert t.shape == series.shape == noisy.shape and np.array_equal(_bits(series), _bits(one)), obs
        # stiffness=None: the parent's path, rsf_law_observe, bit for bit
        model.stiffness, model.observable = None, "mu"
        eng.set_model(model, 1)
        assert eng.stiffness is None
        want = np.asarray(eng.law_observe("slip", "mu", s["dc"], s["a"], s["b"])[1])
        assert np.array_equal(_bits(model.evaluate_batch(s["dc"], s["a"], s["b"])), _bits(want.T))
        assert not np.array_equal(want, np.asarray(eng.stiff_observe("slip", "mu", SC.K_ACC, s["dc"], s["a"], s["b"])[1]))
    finally:
        if model._engine is not None:
            model._engine.close()


# ---- the refusals of the C ABI -------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, gpu_engine):
    """stiffness not finite or not > 0: RSF_ERR_INVALID naming the function; RSF_FLAG_DOP853: RSF_ERR_UNSUPPORTED;
    RSF_FLAG_FP32_SOLVE runs the float64 solve."""
    eng = gpu_engine
    m = C.spec()
    eng.set_model(_model(pkg, m, R.table(m, "step")), 1)
    data = _dr_data("aging", "mu")[0]
    n = 64
    q, l, cnt = np.full((n, 1), 20.0), np.zeros(n), [np.zeros(n, dtype=np.int32) for _ in COUNTERS]
    for bad in (0.0, -4e-3, float("inf"), float("nan")):
        for name, call in (("rsf_stiff_observe", lambda: eng.stiff_observe("aging", "mu", bad, [20.0])),
                           ("rsf_stiff_dr_run", lambda: eng.stiff_dr_run("aging", "mu", bad, q, l, data, 5.0, 200.0, [[1.0]], 1, cnt)),
                           ("rsf_stiff_dr_ssq", lambda: eng.stiff_dr_ssq("aging", "mu", bad, q, np.ones(n, np.uint8), data))):
            with pytest.raises(pkg.RsfError, match=f"{name}: stiffness must be finite and > 0") as ei:
                call()
            assert ei.value.code == -1
    with pytest.raises(pkg.RsfError, match="rsf_stiff_observe: law is RSF_LAW_AGEING"):
        eng.stiff_observe(7, 1, SC.K_ACC, [20.0])
    plain = pkg.RateStateModel(number_time_steps=500)  # the built-in history
    eng.set_model(plain, 1)
    want = np.asarray(eng.stiff_observe("aging", "mu", SC.K_ACC, [20.0, 35.0])[1])
    assert np.isfinite(want).all()
    plain.precision = "float32"
    eng.set_model(plain, 1)
    assert np.array_equal(_bits(eng.stiff_observe("aging", "mu", SC.K_ACC, [20.0, 35.0])[1]), _bits(want))
    plain.precision, plain.integrator = "float64", "dop853"
    eng.set_model(plain, 1)
    for call in (lambda: eng.stiff_observe("aging", "mu", SC.K_ACC, [20.0]),
                 lambda: eng.stiff_dr_run("aging", "mu", SC.K_ACC, q, l, data, 5.0, 200.0, [[1.0]], 1, cnt),
                 lambda: eng.stiff_dr_ssq("aging", "mu", SC.K_ACC, q, np.ones(n, np.uint8), data)):
        with pytest.raises(pkg.RsfError, match="RSF_FLAG_DOP853 is not supported") as ei:
            call()
        assert ei.value.code == -5
