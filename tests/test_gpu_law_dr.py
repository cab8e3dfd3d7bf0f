"""
GPU tests of the delayed-rejection sampler under either state law and any observable (include/rsf_law_dr.h: rsf_law_dr_run /
rsf_law_dr_ssq; Engine.law_dr_run / law_dr_ssq / law_gn_factor / law_dr; MCMC.sample_law):
  1. rsf_law_dr_ssq is rsf_law_observe's SSq, bit for bit, whatever the arrangement;
  2. the fused kernel against the split path through rsf_law_dr_ssq, bit for bit;
  3. Engine.law_dr against Engine.dr_from_ssq on law_ssq_fn, bit for bit;
  4. adaptation is burn-in only;
  5. end to end on friction data, one parameter, held to the quadrature;
  6. end to end, three parameters, both truths;
  7. the refusals through ctypes.
The common problem: nsteps 500 under the step history, truth (Dc, a, b) = (20, 0.011, 0.014), noise 5 % of the excursion
(observe_reference.bf_data); boxes (5, 200) at d = 1 and (8, 0.009, 0.012) .. (60, 0.013, 0.016) at d = 3, in which the CPU
specification's SSq is finite at the corners and at 40 interior points for every observable under both laws; starts
default_rng(7) uniform in [15, 25] x [0.0105, 0.0115] x [0.0135, 0.0145]; the factor law_gn_factor's at the truth; gamma 0.3,
seed 5, offset 900.  The expectation figures quoted below are the CPU specification's (tests/law_dr_reference.py).
"""
import functools

import numpy as np
import pytest

import dr_reference as dr
import law_cases as C
import law_dr_reference as S
import law_reference as R
import observe_cases as OC
import observe_reference as O
import smc_reference as smc

pytestmark = pytest.mark.gpu

COUNTERS = ("accepted1", "accepted2", "outbox1", "outbox2", "stuck")
GAMMA, SEED, OFFSET = 0.3, 5, 900
BOX = {1: (np.array([R.BF_BOX[0]]), np.array([R.BF_BOX[1]])), 3: (S.LO3, S.HI3)}
SENT = -7.25


def _model(pkg, nsteps=500, substeps=1, **attrs):
    m = pkg.RateStateModel(number_time_steps=nsteps)
    m.substeps = substeps
    m.loading = R.step_history
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _bits(x):
    x = np.ascontiguousarray(np.asarray(x.cpu() if hasattr(x, "cpu") else x))
    return x.view(np.int32 if x.dtype.itemsize == 4 else (np.uint8 if x.dtype.itemsize == 1 else np.int64))


def _counters(n):
    return [np.zeros(n, dtype=np.int32) for _ in COUNTERS]


@functools.lru_cache(maxsize=None)
def _data(law, obs, nsteps=500, substeps=1, other=False):
    """the common problem's data; other: the same clean series under another noise draw, a second group's series"""
    m = C.spec(nsteps, substeps)
    vl = R.table(m, "step")
    if not other:
        return O.bf_data(m, vl, law, obs)
    clean = O.forward(m, [R.BF_TRUTH], vl, law, obs)[0][:, 0]
    return clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(R.BF_SEED + 1).standard_normal(clean.size)


def _starts(d, n):
    rng = np.random.default_rng(7)
    q = np.column_stack([rng.uniform(15.0, 25.0, n), rng.uniform(0.0105, 0.0115, n), rng.uniform(0.0135, 0.0145, n)])[:, :d]
    return np.ascontiguousarray(q)


def _gn(eng, law, obs, d, data):
    return eng.law_gn_factor(law, obs, S.TRUTH3[:d], data)[0]


# ---- 1. one stage's SSq is law_observe's -------------------------------------------------------------------------------------------------
def _ssq_against_observe(eng, law, obs, d, n, data, tag):
    """law_dr_ssq at n points of the d-box with every third lane masked out, against law_observe on the compacted masked-in points"""
    lo, hi = BOX[d]
    y = np.ascontiguousarray(lo + (hi - lo) * np.random.default_rng([n, d]).uniform(0.05, 0.95, (n, d)))
    mask = (np.arange(n) % 3 != 2).astype(np.uint8)
    G = 1 if data.ndim == 1 else data.shape[0]
    got = eng.law_dr_ssq(law, obs, y, mask, data, ssq=np.full(n, SENT))
    per = n // G
    for g in range(G):
        rows = np.flatnonzero(mask[g * per:(g + 1) * per]) + g * per
        ab = [np.ascontiguousarray(y[rows, p]) for p in (1, 2)] if d == 3 else [None, None]
        want = eng.law_observe(law, obs, np.ascontiguousarray(y[rows, 0]), ab[0], ab[1], data=data if G == 1 else data[g], want_ssq=True, want_series=False)[0]
        assert np.isfinite(want).all() and (want > 0).all(), tag
        assert np.array_equal(_bits(got[rows]), _bits(want)), (tag, d, n, g)
    assert (got[mask == 0] == SENT).all(), (tag, d, n)


def _non_default():
    """tests/golden/forward_nondefault.json's V_ref, mu_ref, mu_t_zero and k1, the step history as a table in the model's units"""
    attrs = dict(V_ref=1.7, mu_ref=0.55, mu_t_zero=0.58, k1=3e-7)
    return dict(attrs, loading=R.table(C.spec(**attrs), "step"))


@pytest.mark.parametrize("obs", O.OBSERVABLES)
@pytest.mark.parametrize("law", R.LAWS)
def test_stage_ssq_is_law_observe_bit_for_bit(pkg, law, obs):
    data = _data(law, obs)
    with pkg.Engine(mem="host") as eng:
        for tag, attrs in (("damped", {}), ("k1 = 0", dict(k1=0.0)), ("undamped", dict(RadiationDamping=False)), ("non-default", _non_default())):
            eng.set_model(_model(pkg, **attrs), 1)
            for d in (1, 3):
                for n in (1, 63, 65, 133):
                    _ssq_against_observe(eng, law, obs, d, n, data, tag)
        # the table in two chunks
        eng.set_model(_model(pkg, 900, 4), 4)
        assert 2 * 4 * (eng.nout - 1) + 1 + eng.nout > 56 * 1024 // 8
        for d in (1, 3):
            _ssq_against_observe(eng, law, obs, d, 65, _data(law, obs, 900, 4), "two chunks")
    # two groups, each against its own series
    with pkg.Engine(mem="host", block_threads=64) as eng:
        eng.set_model(_model(pkg), 1)
        two = np.stack([data, _data(law, obs, other=True)])
        for d in (1, 3):
            _ssq_against_observe(eng, law, obs, d, 128, two, "two groups")


# ---- 2. fused against split ----------------------------------------------------------------------------------------------------------------
# CPU specification (dr_reference.run on observe_reference.forward), four iterations, first / second stage acceptances of the first
# three cases: 285/144, 156/85, 275/167, which an MI355X reproduced count for count when this was written; there the two series
# gave 127/185 (with 252 outbox1), the two chunks 268/172 and the edge case 258/159 (with 128 outbox1, 64 of them the first wave's
# in iteration 1): far from the conditions below
FUSED_CASES = {
    "ageing, mu, d1, 133 chains": dict(law="aging", obs="mu", d=1, n=133),
    "slip, mu, d3, 81 chains, undamped": dict(law="slip", obs="mu", d=3, n=81, damping=False),
    "slip, acc, d1, 133 chains": dict(law="slip", obs="acc", d=1, n=133),
    "ageing, theta, d3, two series": dict(law="aging", obs="theta", d=3, n=128, groups=2),
    "slip, velocity, d1, two chunks": dict(law="slip", obs="velocity", d=1, n=133, substeps=8),
    "slip, mu, d1, a wave at the edge": dict(law="slip", obs="mu", d=1, n=133, edge=True, block=128),
}


@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_fused_against_split(pkg, name):
    c = FUSED_CASES[name]
    law, obs, d, n, G, B, sub = c["law"], c["obs"], c["d"], c["n"], c.get("groups", 1), c.get("block", 64), c.get("substeps", 1)
    data = _data(law, obs, 500, sub) if G == 1 else np.stack([_data(law, obs, 500, sub), _data(law, obs, 500, sub, other=True)])
    lo, hi = BOX[d]
    shape = 0.5 * data.shape[-1]
    q0 = _starts(d, n)
    model = _model(pkg, 500, sub, RadiationDamping=c.get("damping", True))
    with pkg.Engine(mem="host", block_threads=B) as eng:
        eng.set_model(model, sub)
        assert (2 * sub * (eng.nout - 1) + 1 + eng.nout > 56 * 1024 // 8) == (sub == 8)
        L1 = _gn(eng, law, obs, d, data if G == 1 else data[0])
        L = L1 if G == 1 else np.stack([L1, 2.0 * L1])
        if c.get("edge"):
            # every chain of the first wave sits next to the edge its first proposal of iteration 1 moves towards (the sign of its
            # normal, from the stream), so that in iteration 1 the whole wave skips solve 1 while the other wave of its workgroup solves
            z = smc.normals(SEED, (OFFSET + np.arange(64)).astype(np.uint64), 1, 1)[:, 0]
            q0[:64, 0] = np.where(z > 0, hi[0] - 1e-6, lo[0] + 1e-6)
        per = n // G
        l0 = np.concatenate([-shape * np.log(eng.law_ssq_fn(law, data if G == 1 else data[g], obs)(q0[g * per:(g + 1) * per])) for g in range(G)])
        assert np.isfinite(l0).all()
        fused, split, once = [dict(q=q0.copy(), l=l0.copy(), c=_counters(n)) for _ in range(3)]
        rows = []
        for it in range(1, 5):
            tq, tl = eng.law_dr_run(law, obs, fused["q"], fused["l"], data, lo, hi, L, 1, fused["c"], gamma=GAMMA, shape=shape, seed=SEED, offset=OFFSET,
                                    iter0=it, trace=True)
            kw = dict(gamma=GAMMA, seed=SEED, offset=OFFSET, iteration=it)
            y, m = eng.dr_propose(split["q"], split["l"], lo, hi, L, 1, **kw)
            if c.get("edge") and it == 1:
                assert not m[:64].any() and m[64:128].any()
            s = eng.law_dr_ssq(law, obs, y, m, data)
            l1, pend = eng.dr_accept(split["q"], split["l"], lo, hi, 1, y, m, s, split["c"], shape, **kw)
            y, m = eng.dr_propose(split["q"], split["l"], lo, hi, L, 2, pending=pend, **kw)
            s = eng.law_dr_ssq(law, obs, y, m, data)
            eng.dr_accept(split["q"], split["l"], lo, hi, 2, y, m, s, split["c"], shape, l1=l1, pending=pend, **kw)
            same = {k: bool(np.array_equal(_bits(fused[k]), _bits(split[k]))) for k in ("q", "l")}
            same.update({k: bool(np.array_equal(a, b)) for k, a, b in zip(COUNTERS, fused["c"], split["c"])})
            print(f"{name} iteration {it}: counters { {k: int(v.sum()) for k, v in zip(COUNTERS, fused['c'])} } of {it * n}; bit-identical {same}")
            assert all(same.values()), same
            assert tq[0].tobytes() == fused["q"].tobytes() and tl[0].tobytes() == fused["l"].tobytes()
            rows.append((tq[0].copy(), tl[0].copy()))
        a1, a2, o1, o2, stuck = fused["c"]
        assert a1.sum() > 0 and a2.sum() > 0 and stuck.sum() == 0 and (a1 + a2 <= 4).all() and (a1 + o2 + a2 <= 4).all()
        if c.get("edge"):
            assert (o1[:64] >= 1).all()
        # four iterations inside one launch: the bits of four launches of one, the trace rows too
        tq, tl = eng.law_dr_run(law, obs, once["q"], once["l"], data, lo, hi, L, 4, once["c"], gamma=GAMMA, shape=shape, seed=SEED, offset=OFFSET, iter0=1,
                                trace=True)
        for k in ("q", "l"):
            np.testing.assert_array_equal(_bits(once[k]), _bits(fused[k]), err_msg=k)
        for k, a, b in zip(COUNTERS, once["c"], fused["c"]):
            np.testing.assert_array_equal(a, b, err_msg=k)
        for it in range(4):
            assert tq[it].tobytes() == rows[it][0].tobytes() and tl[it].tobytes() == rows[it][1].tobytes()
    # device memory: the same bits
    import torch

    with pkg.Engine(mem="device", block_threads=B) as dev:
        dev.set_model(model, sub)
        st = dict(q=dev._in(q0), l=dev._in(l0), c=[dev._ints(np.zeros(n)) for _ in COUNTERS])
        tq, tl = dev.law_dr_run(law, obs, st["q"], st["l"], data, lo, hi, L, 4, st["c"], gamma=GAMMA, shape=shape, seed=SEED, offset=OFFSET, iter0=1, trace=True)
        torch.cuda.synchronize()
        for k in ("q", "l"):
            np.testing.assert_array_equal(_bits(st[k]), _bits(fused[k]), err_msg=f"device memory: {k}")
        for k, a, b in zip(COUNTERS, st["c"], fused["c"]):
            np.testing.assert_array_equal(np.asarray(a.cpu()), b, err_msg=f"device memory: {k}")
        assert np.asarray(tq.cpu())[3].tobytes() == fused["q"].tobytes()


# ---- 3. law_dr against dr_from_ssq -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law, d", [("slip", 1), ("aging", 3)])
def test_law_dr_is_dr_from_ssq_bit_for_bit(pkg, law, d):
    n, n_iter = 256, 8
    data = _data(law, "mu")
    lo, hi = BOX[d]
    q0 = _starts(d, n)
    with pkg.Engine(mem="host") as eng:
        eng.set_model(_model(pkg), 1)
        L = _gn(eng, law, "mu", d, data)
        kw = dict(gamma=GAMMA, seed=SEED, offset=OFFSET)
        fused = eng.law_dr(law, "mu", q0, data, lo, hi, L, n_iter, adapt_launches=0, **kw)
        split = eng.dr_from_ssq(eng.law_ssq_fn(law, data, "mu"), q0, lo, hi, L, n_iter, 0.5 * eng.nout, **kw)
    print(f"{law} d {d}: accepted {int(fused.accepted1.sum())} / {int(fused.accepted2.sum())} of {n * n_iter}, outside the box "
          f"{int(fused.outbox1.sum())} / {int(fused.outbox2.sum())}, solves {fused.n_solves}")
    assert fused.iterations.tolist() == split.iterations.tolist() == list(range(1, n_iter + 1))
    for k in ("q", "l", "trace_q", "trace_l"):
        np.testing.assert_array_equal(_bits(getattr(fused, k)), _bits(getattr(split, k)), err_msg=k)
    for k in COUNTERS:
        np.testing.assert_array_equal(getattr(fused, k), getattr(split, k), err_msg=k)
    assert fused.accepted1.sum() > 0 and fused.accepted2.sum() > 0 and fused.stuck.sum() == 0 and fused.n_solves == split.n_solves


# ---- 4. adaptation is burn-in only -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_adaptation_is_burn_in_only(pkg, d):
    law, obs = "slip", "mu"
    data = np.stack([_data(law, obs), _data(law, obs, other=True)])
    lo, hi = BOX[d]
    B, per = 64, 128
    q0 = _starts(d, 2 * per)
    with pkg.Engine(mem="device", block_threads=B) as eng:
        eng.set_model(_model(pkg), 1)
        L1 = _gn(eng, law, obs, d, data[0])
        L0 = np.stack([L1, 0.5 * L1])
        kw = dict(gamma=GAMMA, seed=9, offset=40, iters_per_launch=4)
        whole = eng.law_dr(law, obs, q0, data, lo, hi, L0, 20, keep=8, adapt_launches=3, **kw)
        burn = eng.law_dr(law, obs, q0, data, lo, hi, L0, 12, keep=12, adapt_launches=3, **kw)
        # the factor after the burn-in: the formula on every burn-in state, group by group
        for g in range(2):
            want = dr.adapted_factor(burn.trace_q[:, g * per:(g + 1) * per].reshape(-1, d), lo, hi, L0[g])
            sd = np.sqrt(np.diag(want @ want.T))
            assert (np.abs(burn.chol[g] @ burn.chol[g].T - want @ want.T) / np.outer(sd, sd)).max() < 1e-9
        np.testing.assert_array_equal(whole.chol, burn.chol)
        assert not np.array_equal(whole.chol, L0)
        # the kept part is a frozen run from the burn-in's final state at the same Philox iterations
        tail = eng.law_dr(law, obs, burn.q, data, lo, hi, burn.chol, 8, keep=8, adapt_launches=0, iter0=13, l0=burn.l, **kw)
        # ... and after adapt_launches launches the factor no longer changes
        np.testing.assert_array_equal(tail.chol, burn.chol)
    assert whole.iterations.tolist() == list(range(13, 21)) == tail.iterations.tolist()
    np.testing.assert_array_equal(_bits(tail.trace_q), _bits(whole.trace_q))
    np.testing.assert_array_equal(_bits(tail.trace_l), _bits(whole.trace_l))
    np.testing.assert_array_equal(_bits(tail.q), _bits(whole.q))
    for k in COUNTERS:
        np.testing.assert_array_equal(getattr(burn, k) + getattr(tail, k), getattr(whole, k), err_msg=k)


# ---- 5. end to end, one parameter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("truth", R.LAWS)
def test_sample_law_on_friction_data(pkg, truth):
    """test_sample_dr_on_friction_data's check on the fused path from qstart with factor="gn", adapting in the burn-in: the mean of
    the per-chain means within 4.5 standard errors of the quadrature's mean.  The CPU specification of this construction
    (tests/law_dr_reference.py) gives z = +0.61 (ageing) and +0.13 (slip), acceptance 0.44 / 0.46, pooled SD 0.1273 / 0.1638 against
    the quadrature's 0.1266 / 0.1644."""
    p = OC.friction_problem(truth)
    model = _model(pkg, observable="mu", state_law=truth)
    model.loading = p["vl"]
    mc = pkg.MCMC(model, p["data"], R.BF_TRUTH, ["Uniform", *R.BF_BOX], R.BF_TRUTH, nsamples=10, verbose=False)
    pool = mc.sample_law(256, 200, nburn=96, seed=9)
    x = np.asarray(pool.samples)[:, :, 0]
    assert x.shape == (104, 256) and pool.stats["stuck"] == 0 and pool.stats["adapt"] is True and pool.stats["path"] == "law_dr"
    means = x.mean(axis=0)
    se = means.std(ddof=1) / np.sqrt(means.size)
    z = (means.mean() - p["mean"][truth]) / se
    print(f"truth {truth}: pooled mean {means.mean():.4f}, quadrature {p['mean'][truth]:.4f} (SD {p['sd'][truth]:.4f}), pooled SD {x.std():.4f}, SE {se:.2e}, "
          f"z {z:+.2f}; accept rates {pool.stats['accept_rate1']:.2f} {pool.stats['accept_rate2']:.2f} ({pool.accept_rate:.2f}); adapted factor "
          f"{float(pool.stats['chol'][0, 0, 0]):.4f}")
    assert 0.05 < pool.accept_rate < 0.95
    assert abs(z) < 4.5
    # the chains' l is the friction's under the true law: -N/2 log SSq of law_observe at the final states
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        ssq = eng.law_ssq_fn(truth, p["data"], observable="mu")(x[-1].reshape(-1, 1))
    assert np.allclose(pool.stats["l"][-1], -0.5 * len(p["data"]) * np.log(ssq), rtol=1e-12, atol=0.0)


# ---- 6. end to end, three parameters -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("truth", R.LAWS)
def test_sample_law_three_parameters(pkg, truth):
    """(Dc, a, b) from friction data under the true law, from the truth with factor="gn".  There is no quadrature at d = 3 under a law:
    exactness rests on test 3's bit identity with the split path, which is held to closed-form targets (tests/test_gpu_dr.py).
    Sanity bounds from the CPU specification of this construction: pooled SD over law_gn_factor's Laplace SD in [0.9, 1.1] per
    parameter (the specification: 0.985 to 1.031; the Monte Carlo error of the ratio at this size is about 1 %); |pooled mean -
    truth| < 4 pooled SD (the specification's largest: 1.78); acceptance in (0.05, 0.95) (0.31 at stage 1, 0.53 at stage 2)."""
    p = OC.friction_problem(truth)
    model = _model(pkg, observable="mu", state_law=truth)
    model.loading = p["vl"]
    priors = [["Uniform", float(a), float(b)] for a, b in zip(S.LO3, S.HI3)]
    mc = pkg.MCMC(model, p["data"], R.BF_TRUTH, priors, S.TRUTH3.copy(), nsamples=10, verbose=False)
    pool = mc.sample_law(256, 400, nburn=192, seed=9)
    x = np.asarray(pool.samples).reshape(-1, 3)
    assert pool.samples.shape == (208, 256, 3) and pool.stats["stuck"] == 0 and pool.stats["adapt"] is True
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        _, cov, _ = eng.law_gn_factor(truth, "mu", S.TRUTH3, p["data"])
    laplace = np.sqrt(np.diag(cov))
    sd, mean = x.std(axis=0), x.mean(axis=0)
    print(f"truth {truth}: pooled mean {mean}, pooled SD {sd}, Laplace SD {laplace}, ratio {sd / laplace}, (mean - truth) / SD {(mean - S.TRUTH3) / sd}; "
          f"accept rates {pool.stats['accept_rate1']:.2f} {pool.stats['accept_rate2']:.2f} ({pool.accept_rate:.2f})")
    assert ((sd / laplace > 0.9) & (sd / laplace < 1.1)).all()
    assert (np.abs(mean - S.TRUTH3) < 4.0 * sd).all()
    assert 0.05 < pool.accept_rate < 0.95


# ---- 7. the refusals through ctypes ----------------------------------------------------------------------------------------------------------
def _plain(pkg, **attrs):
    m = pkg.RateStateModel(number_time_steps=500)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _state(n, d=1, l=0.0):
    q = np.ascontiguousarray(np.linspace(900.0, 1100.0, n * d).reshape(n, d))
    return dict(q=q, l=np.full(n, float(l)), c=_counters(n))


def test_refusals(pkg):
    P = lambda x: x.ctypes.data
    dp = lambda v: np.atleast_1d(np.asarray(v, dtype=np.float64)).ctypes.data_as(pkg._abi._DP)
    with pkg.Engine(mem="host", block_threads=64) as eng:
        lib, ctx = eng.lib, eng._ctx
        st, zeros, ones, mask = _state(128), np.zeros(500), np.ones(128), np.ones(128, np.uint8)
        run = lambda s, law=1, obs=1: [ctx, law, obs, 128, 1, P(s["q"]), P(s["l"]), P(zeros), 1, dp(0.0), dp(1e4), dp(1.0), 0.2, 2, 250.0, 0, 0, 1, 1] + \
            [P(c) for c in s["c"]] + [None, None]
        ssq = lambda law=1, obs=1: [ctx, law, obs, 128, 1, P(st["q"]), P(mask), P(zeros), 1, P(ones)]
        # no model
        assert lib.rsf_law_dr_run(*run(st)) == -3 and b"rsf_law_dr_run" in lib.rsf_last_error()
        assert lib.rsf_law_dr_ssq(*ssq()) == -3 and b"rsf_law_dr_ssq" in lib.rsf_last_error()
        eng.set_model(_plain(pkg), 1)
        ok = run(st)
        assert lib.rsf_law_dr_run(*ok) == 0 and lib.rsf_law_dr_ssq(*ssq()) == 0
        # the law and the observable: rsf_law_observe's messages
        for law in (-1, 2, 7):
            assert lib.rsf_law_dr_run(*run(st, law=law)) == -1 and b"rsf_law_dr_run: law is RSF_LAW_AGEING" in lib.rsf_last_error()
            assert lib.rsf_law_dr_ssq(*ssq(law=law)) == -1 and b"rsf_law_dr_ssq: law is RSF_LAW_AGEING" in lib.rsf_last_error()
        for obs in (-1, 4):
            assert lib.rsf_law_dr_run(*run(st, obs=obs)) == -1 and b"rsf_law_dr_run: observable is RSF_OBS_ACC" in lib.rsf_last_error()
            assert lib.rsf_law_dr_ssq(*ssq(obs=obs)) == -1 and b"rsf_law_dr_ssq: observable is RSF_OBS_ACC" in lib.rsf_last_error()
        # every argument error of rsf_dr_run, under this function's name (the arguments lie two places further on)
        for i, v in ((3, 0), (4, 2), (4, 4), (5, None), (6, None), (7, None), (8, 0), (8, 65), (9, None), (10, None), (11, None), (11, dp(0.0)), (11, dp(-1.0)),
                     (11, dp(np.inf)), (11, dp(np.nan)), (12, 0.0), (12, 1.5), (12, np.nan), (13, 0), (13, 3), (14, 0.0), (14, np.nan), (16, -1), (17, 0),
                     (17, 2 ** 32), (18, 0), (18, 65), (19, None), (20, None), (21, None), (22, None), (23, None), (24, P(st["q"])), (25, P(st["l"]))):
            bad = list(ok)
            bad[i] = v
            assert lib.rsf_law_dr_run(*bad) == -1, i
            assert b"rsf_law_dr_run" in lib.rsf_last_error(), i
        assert lib.rsf_law_dr_run(None, *ok[1:]) == -1 and b"rsf_law_dr_run" in lib.rsf_last_error()
        bad = list(ok)
        bad[9], bad[10] = dp(5.0), dp(5.0)
        assert lib.rsf_law_dr_run(*bad) == -1
        st3 = _state(128, 3)
        L3 = [1.0, 0.5, 1.0, 0.5, 0.5, 1.0]
        ok3 = [ctx, 1, 1, 128, 3, P(st3["q"]), P(st3["l"]), P(zeros), 1, dp([0.0] * 3), dp([1e4] * 3), dp(L3), 0.2, 2, 250.0, 0, 0, 1, 1] + \
            [P(c) for c in st3["c"]] + [None, None]
        assert lib.rsf_law_dr_run(*ok3) == 0
        for e, v in ((0, 0.0), (2, -1.0), (5, np.inf), (3, np.nan)):  # a diagonal entry not positive and finite; an entry not finite
            bad = list(ok3)
            bad[11] = dp([v if k == e else x for k, x in enumerate(L3)])
            assert lib.rsf_law_dr_run(*bad) == -1, e
        # groups in whole workgroups
        two, st192, st256 = np.zeros((2, 500)), _state(192), _state(256)
        grp = lambda s, n: [ctx, 1, 1, n, 1, P(s["q"]), P(s["l"]), P(two), 2, dp(0.0), dp(1e4), dp([1.0, 1.0]), 0.2, 2, 250.0, 0, 0, 1, 1] + \
            [P(c) for c in s["c"]] + [None, None]
        assert lib.rsf_law_dr_run(*grp(st192, 192)) == -1 and lib.rsf_law_dr_run(*grp(st256, 256)) == 0
        # rsf_dr_ssq's
        for i, v in ((3, 0), (4, 2), (5, None), (6, None), (7, None), (8, 0), (9, None)):
            bad = ssq()
            bad[i] = v
            assert lib.rsf_law_dr_ssq(*bad) == -1, i
            assert b"rsf_law_dr_ssq" in lib.rsf_last_error(), i
        # the integrator
        eng.set_model(_plain(pkg, integrator="dop853"), 1)
        assert lib.rsf_law_dr_run(*run(st)) == -5 and b"rsf_law_dr_run" in lib.rsf_last_error()
        assert lib.rsf_law_dr_ssq(*ssq()) == -5 and b"rsf_law_dr_ssq" in lib.rsf_last_error()
        # a float32-flagged default model gets the float64 solve: the bits of the float64 model
        data = np.cos(np.linspace(0.0, 3.0, 500))
        out = []
        for attrs in (dict(precision="float32"), dict()):
            eng.set_model(_plain(pkg, **attrs), 1)
            s = _state(128, l=-1e9)  # far below any l': the first proposals inside the box are accepted, so the solve's bits reach l
            eng.law_dr_run("aging", "acc", s["q"], s["l"], data, 0.0, 1e4, [[30.0]], 2, s["c"], gamma=0.2, shape=250.0)
            out.append(s)
        for k in ("q", "l"):
            np.testing.assert_array_equal(_bits(out[0][k]), _bits(out[1][k]), err_msg=k)
        assert out[1]["c"][0].sum() > 0 and (out[1]["l"] > -1e9).any()
