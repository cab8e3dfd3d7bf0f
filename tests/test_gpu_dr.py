"""
GPU tests of the two-stage delayed-rejection sampler (include/rsf_dr.h: rsf_dr_run / _propose / _accept / _ssq; Engine.dr,
Engine.dr_from_ssq, MCMC.sample_dr, RSF.inference_dr):
  1. the split path against the NumPy specification (tests/dr_reference.py), with rows crafted for every way an iteration ends;
  2. the fused kernel against the split path through rsf_dr_ssq on the real model, bit for bit;
  3. stages = 1 against rsf_smc_move at beta = 1, bit for bit;
  4. the target: the closed forms through the split path and the real model through the fused kernel, held to the quadrature;
  5. the bad start of the reference's own problem (Dc_true = 100, every chain at 1000);
  6. adaptation is burn-in only;
  7. the refusals;
  8. the front ends.
"""
import numpy as np
import pytest

import dr_cases as cases
import dr_reference as dr
import posterior_reference as R
import smc_reference as smc
from conftest import synthetic_data
from test_gpu_posterior import BOX1, HI3, LO3, _reference

pytestmark = pytest.mark.gpu

TIE = 1e-9
EPS = 2.0 ** -52
COUNTERS = ("accepted1", "accepted2", "outbox1", "outbox2", "stuck")
_CACHE = {}


def _model(pkg, nsteps=500, damping=True):
    m = pkg.RateStateModel(number_time_steps=nsteps)
    m.RadiationDamping = damping
    return m


def _bits(x):
    x = np.ascontiguousarray(np.asarray(x.cpu() if hasattr(x, "cpu") else x))
    return x.view(np.int32 if x.dtype.itemsize == 4 else (np.uint8 if x.dtype.itemsize == 1 else np.int64))


def _counters(n):
    return [np.zeros(n, dtype=np.int32) for _ in COUNTERS]


# ---- 1. the split path against the specification ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3])
def test_split_path_against_the_specification(pkg, d):
    prob = cases.split_problem(d)
    lo, hi, L, shape, fn, fix = (prob[k] for k in ("lo", "hi", "L", "shape", "fn", "fix"))
    gamma, seed, offset = cases.SPLIT_GAMMA, cases.SPLIT_SEED, cases.SPLIT_OFFSET
    q = prob["q0"].copy()
    n = q.shape[0]
    l = dr.start_l(q, fn, shape)
    for r, v in prob["bad_l"].items():
        l[r] = v
    cnt, want_cnt = _counters(n), dr.new_counters(n)
    crafted = np.arange(cases.SPLIT_N, n)
    in_band, smallest, steps = np.zeros(n, bool), np.inf, []
    bound = 4 * EPS * (hi - lo)  # a few ulp of the box width: y = q + L z, three terms of at most the width each

    def solved(stage, y, mask):
        s = np.ones(n)
        if mask.any():
            s[mask] = fn(y[mask])
        return fix(stage, s)

    with pkg.Engine(mem="host", block_threads=64) as eng:
        for it in range(1, cases.SPLIT_ITERS + 1):
            # the specification on the GPU's own state of this iteration
            sq, sl = q.copy(), l.copy()
            st = dr.step(sq, sl, fn, lo, hi, L, gamma, 2, shape, seed, offset, it, want_cnt, fix=fix)
            steps.append(st)
            kw = dict(gamma=gamma, seed=seed, offset=offset, iteration=it)
            q_before, l_before = q.copy(), l.copy()
            y1, m1 = eng.dr_propose(q, l, lo, hi, L, 1, **kw)
            m1 = m1.astype(bool)
            assert (np.abs(y1 - st["y1"]) <= bound).all(), np.abs(y1 - st["y1"]).max(axis=0) / (hi - lo)
            np.testing.assert_array_equal(m1, st["in1"])
            np.testing.assert_array_equal(_bits(y1[st["stuck"]]), _bits(q[st["stuck"]]))
            s1 = solved(1, y1, m1)
            l1, pend = eng.dr_accept(q, l, lo, hi, 1, y1, m1, s1, cnt, shape, **kw)
            band1 = st["in1"] & (np.abs(st["margin1"]) <= TIE)
            acc1 = (_bits(q) != _bits(q_before)).any(axis=1) | (_bits(l) != _bits(l_before))
            ok = ~band1
            np.testing.assert_array_equal(acc1[ok], st["acc1"][ok])
            np.testing.assert_array_equal(pend.astype(bool)[ok], st["pending"][ok])
            np.testing.assert_array_equal(np.isneginf(l1), np.isneginf(st["l1"]))
            # l1 is -shape log of the SSq supplied: the device's logarithm and NumPy's are each within an ulp, the product rounds once
            want_l1 = smc.log_target(s1[m1], shape, np.float64)
            fin = np.isfinite(want_l1)
            assert (np.abs(l1[m1][fin] - want_l1[fin]) <= 4 * EPS * np.abs(want_l1[fin])).all()
            # accepted states carry the supplied bits
            np.testing.assert_array_equal(_bits(q[acc1]), _bits(y1[acc1]))
            np.testing.assert_array_equal(_bits(l[acc1]), _bits(l1[acc1]))
            same = ok & st["pending"]  # the chains both sides take into stage 2 from the same state
            q_mid, l_mid = q.copy(), l.copy()
            y2, m2 = eng.dr_propose(q, l, lo, hi, L, 2, pending=pend, **kw)
            m2 = m2.astype(bool)
            assert (np.abs(y2 - st["y2"])[same] <= bound).all()
            np.testing.assert_array_equal(m2[same], st["in2"][same])
            assert not m2[~pend.astype(bool)].any() and np.array_equal(_bits(y2[~pend.astype(bool)]), _bits(q[~pend.astype(bool)]))
            s2 = solved(2, y2, m2)
            eng.dr_accept(q, l, lo, hi, 2, y2, m2, s2, cnt, shape, l1=l1, pending=pend, **kw)
            band2 = st["in2"] & ~st["rejected2"] & (np.abs(st["margin2"]) <= TIE)
            acc2 = (_bits(q) != _bits(q_mid)).any(axis=1) | (_bits(l) != _bits(l_mid))
            ok2 = same & ~band2
            np.testing.assert_array_equal(acc2[ok2], st["acc2"][ok2])
            assert not acc2[~pend.astype(bool)].any()
            np.testing.assert_array_equal(_bits(q[acc2]), _bits(y2[acc2]))
            assert (np.abs(l[acc2] - smc.log_target(s2[acc2], shape, np.float64)) <= 4 * EPS * np.abs(l[acc2])).all()
            in_band |= band1 | band2
            for m, w in ((st["margin1"], st["in1"]), (st["margin2"], st["in2"] & ~st["rejected2"])):
                v = np.abs(m[w])
                v = v[np.isfinite(v)]
                smallest = min(smallest, v.min()) if v.size else smallest
        print(f"d {d}: smallest |log alpha - log U| {smallest:.3e}; chains inside the tie band {int(in_band.sum())}; counters "
              f"{ {k: int(c.sum()) for k, c in zip(COUNTERS, cnt)} }")
        assert not in_band[crafted].any()
        assert cases.split_coverage(d, steps, prob) == []
        for k, c in zip(COUNTERS, cnt):
            np.testing.assert_array_equal(c[~in_band], want_cnt[k][~in_band], err_msg=k)
        if not in_band.any():
            assert dr.n_solves(cases.SPLIT_ITERS, dict(zip(COUNTERS, cnt))) == sum(int(s["in1"].sum() + s["in2"].sum()) for s in steps)


# ---- 2. fused against split on the real model --------------------------------------------------------------------------------------------
def _observations(pkg, cpu_engine, truths, substeps):
    key = ("obs", tuple(truths), substeps)
    if key not in _CACHE:
        cpu_engine.set_model(_model(pkg), substeps)
        rows = []
        for k, dc in enumerate(truths):
            truth = np.asarray(cpu_engine.forward([dc])[1])[:, 0]
            rows.append(truth + 0.01 * np.abs(truth).max() * np.random.default_rng(k + 1).standard_normal(truth.size))
        _CACHE[key] = np.ascontiguousarray(rows)
    return _CACHE[key]


FLO, FHI = np.array([600.0, 0.009, 0.013]), np.array([1600.0, 0.013, 0.017])


def _chains(d, n, seed):
    rng = np.random.default_rng(seed)
    q = np.column_stack([rng.uniform(700.0, 1500.0, n), rng.uniform(0.0095, 0.0125, n), rng.uniform(0.0135, 0.0165, n)])[:, :d]
    return np.ascontiguousarray(q)


def _factor(d, scale=1.0):
    return scale * np.diag([25.0, 2e-4, 2e-4][:d]) + (np.array([[0, 0, 0], [-2e-4, 0, 0], [1e-4, 5e-5, 0]])[:d, :d] if d == 3 else 0.0)


FUSED_CASES = {
    "d1, 133 chains": dict(d=1, n=133, damping=True, groups=1, substeps=1),
    "d3, 81 chains, undamped": dict(d=3, n=81, damping=False, groups=1, substeps=1),
    "d1, a wave at the edge": dict(d=1, n=133, damping=False, groups=1, substeps=1, edge=True, block=128),
    "d3, two series": dict(d=3, n=128, damping=True, groups=2, substeps=1),
    "d1, two chunks": dict(d=1, n=133, damping=True, groups=1, substeps=8),
}


@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_fused_against_split_on_the_real_model(pkg, cpu_engine, name):
    c = FUSED_CASES[name]
    d, n, G, B, gamma, seed, offset = c["d"], c["n"], c["groups"], c.get("block", 64), 0.3, 5, 900
    data = _observations(pkg, cpu_engine, (1000.0, 1200.0)[:G], c["substeps"])
    data = data[0] if G == 1 else data
    lo, hi = FLO[:d], FHI[:d]
    shape = 0.5 * data.shape[-1]
    q0 = _chains(d, n, 7)
    L = _factor(d) if G == 1 else np.stack([_factor(d), _factor(d, 2.0)])
    if c.get("edge"):
        # every chain of the first wave sits next to the edge its first proposal of iteration 1 moves towards (the sign of its
        # normal, from the stream), so that in iteration 1 the whole wave skips solve 1 while the other wave of its workgroup solves
        z = smc.normals(seed, (offset + np.arange(64)).astype(np.uint64), 1, 1)[:, 0]
        q0[:64, 0] = np.where(z > 0, 1600.0 - 1e-6, 600.0 + 1e-6)
    with pkg.Engine(mem="host", block_threads=B) as eng:
        eng.set_model(_model(pkg, damping=c["damping"]), c["substeps"])
        per = n // G
        l0 = np.concatenate([-shape * np.log(np.asarray(eng.fit_normal(q0[g * per:(g + 1) * per], data if G == 1 else data[g])[0])) for g in range(G)])
        fused, split, once = [dict(q=q0.copy(), l=l0.copy(), c=_counters(n)) for _ in range(3)]
        rows = []
        for it in range(1, 5):
            tq, tl = eng.dr_run(fused["q"], fused["l"], data, lo, hi, L, 1, fused["c"], gamma=gamma, shape=shape, seed=seed, offset=offset, iter0=it, trace=True)
            kw = dict(gamma=gamma, seed=seed, offset=offset, iteration=it)
            y, m = eng.dr_propose(split["q"], split["l"], lo, hi, L, 1, **kw)
            if c.get("edge") and it == 1:
                assert not m[:64].any() and m[64:].any()
            s = eng.dr_ssq(y, m, data)
            l1, pend = eng.dr_accept(split["q"], split["l"], lo, hi, 1, y, m, s, split["c"], shape, **kw)
            y, m = eng.dr_propose(split["q"], split["l"], lo, hi, L, 2, pending=pend, **kw)
            s = eng.dr_ssq(y, m, data)
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
        tq, tl = eng.dr_run(once["q"], once["l"], data, lo, hi, L, 4, once["c"], gamma=gamma, shape=shape, seed=seed, offset=offset, iter0=1, trace=True)
        for k in ("q", "l"):
            np.testing.assert_array_equal(_bits(once[k]), _bits(fused[k]), err_msg=k)
        for k, a, b in zip(COUNTERS, once["c"], fused["c"]):
            np.testing.assert_array_equal(a, b, err_msg=k)
        for it in range(4):
            assert tq[it].tobytes() == rows[it][0].tobytes() and tl[it].tobytes() == rows[it][1].tobytes()
    # device memory: the same bits
    import torch

    with pkg.Engine(mem="device", block_threads=B) as dev:
        dev.set_model(_model(pkg, damping=c["damping"]), c["substeps"])
        st = dict(q=dev._in(q0), l=dev._in(l0), c=[dev._ints(np.zeros(n)) for _ in COUNTERS])
        tq, tl = dev.dr_run(st["q"], st["l"], data, lo, hi, L, 4, st["c"], gamma=gamma, shape=shape, seed=seed, offset=offset, iter0=1, trace=True)
        torch.cuda.synchronize()
        for k in ("q", "l"):
            np.testing.assert_array_equal(_bits(st[k]), _bits(fused[k]), err_msg=f"device memory: {k}")
        for k, a, b in zip(COUNTERS, st["c"], fused["c"]):
            np.testing.assert_array_equal(np.asarray(a.cpu()), b, err_msg=f"device memory: {k}")
        assert np.asarray(tq.cpu())[3].tobytes() == fused["q"].tobytes()


# ---- 3. one stage is rsf_smc_move at beta = 1 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_one_stage_is_smc_move_bit_for_bit(pkg, cpu_engine, d):
    n, seed, offset = 1037, 12, 77
    data = _observations(pkg, cpu_engine, (1000.0,), 1)[0]
    lo, hi = FLO[:d], FHI[:d]
    q0, L = _chains(d, n, 3), _factor(d, 2.0)
    q0[:8, 0] = np.linspace(1599.0, 1599.9, 8)  # next to the edge: some proposals leave
    with pkg.Engine(mem="host") as eng:
        eng.set_model(_model(pkg), 1)
        shape = 0.5 * eng.nout
        l0 = -shape * np.log(np.asarray(eng.fit_normal(q0, data)[0]))
        qs, ls, acc = eng.smc_move(q0, l0, data, lo, hi, L, 1.0, seed=seed, offset=offset, iter0=1, steps=3)
        q, l, cnt = q0.copy(), l0.copy(), _counters(n)
        eng.dr_run(q, l, data, lo, hi, L, 3, cnt, gamma=0.2, stages=1, seed=seed, offset=offset, iter0=1)
    print(f"d {d}: accepted {int(acc.sum())} of {3 * n}, outside the box {int(cnt[2].sum())}")
    np.testing.assert_array_equal(_bits(q), _bits(qs))
    np.testing.assert_array_equal(_bits(l), _bits(ls))
    assert int(cnt[0].sum()) == int(acc.sum()) > 0 and cnt[2].sum() > 0 and cnt[1].sum() == 0 and cnt[3].sum() == 0 and cnt[4].sum() == 0


# ---- 4. the target -----------------------------------------------------------------------------------------------------------------------
def _held_to_target(tag, ref, res, eng, fails):
    zmax = kmax = 0.0
    for row, it in enumerate(res.iterations):
        std2 = eng.smc_std2(res.trace_l[row], res.shape, res.seed, res.offset, int(it))
        z, k = R.check(f"{tag} iteration {it}", ref, res.trace_q[row], np.asarray(std2.cpu() if hasattr(std2, "cpu") else std2), fails)
        zmax, kmax = max(zmax, z), max(kmax, k)
    first, second = res.accept_rates
    print(f"{tag}: largest |z| {zmax:.2f}, sqrt(C) D {kmax:.2f}; stage 1 accepted {first:.3f}, stage 2 {second:.3f} of its proposals; outside the box "
          f"{res.outbox_rates[0]:.3f} / {res.outbox_rates[1]:.3f}; solves {res.n_solves}")


@pytest.mark.parametrize("d,scale,gamma", cases.LEGS)
def test_closed_form_targets_through_the_split_path(gpu_engine, d, scale, gamma):
    ref, fn, c = cases.closed_reference(d)
    q0 = ref.draw(np.random.default_rng([cases.SEED, d, int(10 * scale)]), cases.C_TARGET)
    cps = cases.CHECKPOINTS
    res = gpu_engine.dr_from_ssq(cases.rows_fn(fn, d), q0, c["lo"], c["hi"], cases.closed_factor(c, scale), max(cps), c["shape"], gamma=gamma,
                                 seed=cases.SEED, keep=max(cps) - min(cps) + 1, thin=max(cps) - min(cps))
    assert res.iterations.tolist() == list(cps)
    fails = []
    _held_to_target(f"closed d {d} scale {scale} gamma {gamma}", ref, res, gpu_engine, fails)
    assert res.stuck.sum() == 0 and res.accepted1.sum() > 0 and res.accepted2.sum() > 0
    assert not fails, fails


@pytest.mark.parametrize("d", [1, 3])
def test_real_model_targets(pkg, cpu_engine, d):
    lo, hi = (BOX1[0], BOX1[1]) if d == 1 else (LO3, HI3)
    ref, data = _reference(pkg, cpu_engine, d, lo, hi)
    q0 = ref.draw(np.random.default_rng(71 + d), 65536)
    L = 3.0 * np.linalg.cholesky(np.atleast_2d(np.cov(q0.T)))  # deliberately wide: three posterior standard deviations
    fails = []
    with pkg.Engine(mem="device") as eng:
        eng.set_model(_model(pkg), 1)
        res = eng.dr(q0, data, lo, hi, L, 8, gamma=0.2, seed=41 + d, keep=5, thin=4, iters_per_launch=4)
        assert res.iterations.tolist() == [4, 8]
        _held_to_target(f"real d {d}", ref, res, eng, fails)
    assert res.stuck.sum() == 0 and res.accepted1.sum() > 0 and res.accepted2.sum() > 0
    assert not fails, fails


# ---- 5. the bad start --------------------------------------------------------------------------------------------------------------------
def test_the_bad_start_of_the_reference_problem(pkg, cpu_engine):
    """Dc_true = 100 in the box (0, 1e4), every chain started at 1000 with the init kernel's factor and no adaptation"""
    cpu_engine.set_model(_model(pkg), 1)
    data = synthetic_data(cpu_engine, dc_true=100.0)
    ref = R.Posterior1(R.checker_ssq(cpu_engine, data), BOX1[0], BOX1[1], 0.5 * data.size)
    q_lo, q_hi = ref.marg["Dc"].quantiles((0.005, 0.995))
    mc = pkg.MCMC(_model(pkg), data, 100.0, ["Uniform", BOX1[0], BOX1[1]], 1000.0)
    n, n_iter = 512, 400
    pool = mc.sample_dr(n, n_iter, nburn=200, start="qstart", factor="init", adapt=False, seed=3)
    s = pool.stats
    med = float(np.median(pool.samples[-1]))
    print(f"bad start: first proposals outside the box {s['out_of_bounds'] / (n * n_iter):.3f}, stage 1 accepted {s['accepted1']}, stage 2 accepted "
          f"{s['accepted2']} (rates {s['accept_rate1']:.4f} / {s['accept_rate2']:.4f}), solves {s['n_solves']} for {n * n_iter} iterations; the pool's "
          f"median Dc after the run {med:.2f}, the quadrature's central 99 % interval ({q_lo:.2f}, {q_hi:.2f})")
    assert s["out_of_bounds"] > 0.3 * n * n_iter
    assert s["accepted2"] > s["accepted1"]
    assert s["stuck"] == 0 and s["n_solves"] == (n * n_iter - s["out_of_bounds"]) + (n * n_iter - s["accepted1"] - s["out_of_bounds2"])
    assert q_lo < med < q_hi
    assert pool.samples.shape == (200, n, 1) and np.isfinite(pool.std2).all()


# ---- 6. adaptation is burn-in only ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_adaptation_is_burn_in_only(pkg, cpu_engine, d):
    data = _observations(pkg, cpu_engine, (1000.0, 1200.0), 1)
    lo, hi = FLO[:d], FHI[:d]
    B, per = 64, 128
    q0 = _chains(d, 2 * per, 21)
    L0 = np.stack([_factor(d), _factor(d, 0.5)])
    with pkg.Engine(mem="device", block_threads=B) as eng:
        eng.set_model(_model(pkg), 1)
        kw = dict(gamma=0.3, seed=9, offset=40, iters_per_launch=4)
        whole = eng.dr(q0, data, lo, hi, L0, 20, keep=8, adapt_launches=3, **kw)
        burn = eng.dr(q0, data, lo, hi, L0, 12, keep=12, adapt_launches=3, **kw)
        # the factor after the burn-in: the formula on every burn-in state, group by group
        for g in range(2):
            want = dr.adapted_factor(burn.trace_q[:, g * per:(g + 1) * per].reshape(-1, d), lo, hi, L0[g])
            sd = np.sqrt(np.diag(want @ want.T))
            assert (np.abs(burn.chol[g] @ burn.chol[g].T - want @ want.T) / np.outer(sd, sd)).max() < 1e-9
        np.testing.assert_array_equal(whole.chol, burn.chol)
        assert not np.array_equal(whole.chol, L0)
        # the kept part is a frozen run from the burn-in's final state at the same Philox iterations
        tail = eng.dr(burn.q, data, lo, hi, burn.chol, 8, keep=8, adapt_launches=0, iter0=13, l0=burn.l, **kw)
    assert whole.iterations.tolist() == list(range(13, 21)) == tail.iterations.tolist()
    np.testing.assert_array_equal(_bits(tail.trace_q), _bits(whole.trace_q))
    np.testing.assert_array_equal(_bits(tail.trace_l), _bits(whole.trace_l))
    np.testing.assert_array_equal(_bits(tail.q), _bits(whole.q))
    for k in COUNTERS:
        np.testing.assert_array_equal(getattr(burn, k) + getattr(tail, k), getattr(whole, k), err_msg=k)


# ---- 7. the refusals -----------------------------------------------------------------------------------------------------------------------
def _code(pkg, call):
    with pytest.raises(pkg.RsfError) as ei:
        call()
    return ei.value.code


def _state(n, d=1, l=0.0):
    q = np.ascontiguousarray(np.linspace(900.0, 1100.0, n * d).reshape(n, d))
    return dict(q=q, l=np.full(n, float(l)), c=_counters(n))


def _run(eng, st, **kw):
    a = dict(data=np.zeros(500), lo=BOX1[0], hi=BOX1[1], chol=np.eye(st["q"].shape[1]), n_iter=1, gamma=0.2, stages=2, shape=250.0, seed=0, offset=0, iter0=1)
    a.update(kw)
    return eng.dr_run(st["q"], st["l"], a.pop("data"), a.pop("lo"), a.pop("hi"), a.pop("chol"), a.pop("n_iter"), st["c"], **a)


def test_error_state_without_a_model(pkg):
    with pkg.Engine(mem="host", block_threads=64) as eng:
        assert _code(pkg, lambda: _run(eng, _state(128))) == -3
        assert _code(pkg, lambda: eng.dr_ssq(np.ones((128, 1)), np.ones(128, np.uint8), np.zeros(500))) == -3
        P = lambda x: x.ctypes.data
        dp = lambda v: np.array([v], dtype=np.float64).ctypes.data_as(pkg._abi._DP)
        st, zeros, ones, mask = _state(128), np.zeros(500), np.ones(128), np.ones(128, np.uint8)
        args = [eng._ctx, 128, 1, P(st["q"]), P(st["l"]), P(zeros), 1, dp(0.0), dp(1e4), dp(1.0), 0.2, 2, 250.0, 0, 0, 1, 1] + [P(c) for c in st["c"]] + [None, None]
        assert eng.lib.rsf_dr_run(*args) == -3
        assert eng.lib.rsf_dr_ssq(eng._ctx, 128, 1, P(st["q"]), P(mask), P(zeros), 1, P(ones)) == -3


def test_error_invalid_arguments(pkg):
    P = lambda x: x.ctypes.data
    dp = lambda v: np.atleast_1d(np.asarray(v, dtype=np.float64)).ctypes.data_as(pkg._abi._DP)
    with pkg.Engine(mem="host", block_threads=64) as eng:
        eng.set_model(_model(pkg), 1)
        st = _state(128)
        _run(eng, st)
        _run(eng, _state(100))  # one group: any number of chains
        for kw in (dict(n_iter=0), dict(n_iter=65), dict(iter0=0), dict(iter0=2 ** 32), dict(offset=-1), dict(gamma=0.0), dict(gamma=1.5), dict(gamma=np.nan),
                   dict(gamma=-0.2), dict(stages=0), dict(stages=3), dict(shape=0.0), dict(shape=np.nan), dict(lo=5.0, hi=5.0), dict(hi=np.inf)):
            assert _code(pkg, lambda: _run(eng, st, **kw)) == -1, kw
        two = np.zeros((2, 500))
        assert _code(pkg, lambda: _run(eng, _state(192), data=two, chol=np.ones((2, 1, 1)))) == -1  # 96 chains per series: not whole workgroups
        assert _code(pkg, lambda: _run(eng, _state(129), data=two, chol=np.ones((2, 1, 1)))) == -1
        _run(eng, _state(256), data=two, chol=np.ones((2, 1, 1)))
        lib, ctx, zeros, ones = eng.lib, eng._ctx, np.zeros(500), np.ones(128)
        ok = [ctx, 128, 1, P(st["q"]), P(st["l"]), P(zeros), 1, dp(0.0), dp(1e4), dp(1.0), 0.2, 2, 250.0, 0, 0, 1, 1] + [P(c) for c in st["c"]] + [None, None]
        assert lib.rsf_dr_run(*ok) == 0
        for i, v in ((1, 0), (2, 2), (2, 4), (3, None), (4, None), (5, None), (6, 0), (6, 65), (7, None), (8, None), (9, None), (9, dp(0.0)), (9, dp(-1.0)),
                     (9, dp(np.inf)), (9, dp(np.nan)), (17, None), (18, None), (19, None), (20, None), (21, None), (22, P(st["q"])), (23, P(st["l"]))):
            bad = list(ok)
            bad[i] = v
            assert lib.rsf_dr_run(*bad) == -1, i
        assert lib.rsf_dr_run(None, *ok[1:]) == -1
        st3 = _state(128, 3)
        L3 = [1.0, 0.5, 1.0, 0.5, 0.5, 1.0]
        ok3 = [ctx, 128, 3, P(st3["q"]), P(st3["l"]), P(zeros), 1, dp([0.0] * 3), dp([1e4] * 3), dp(L3), 0.2, 2, 250.0, 0, 0, 1, 1] + [P(c) for c in st3["c"]] + [None, None]
        assert lib.rsf_dr_run(*ok3) == 0
        for e, v in ((0, 0.0), (2, -1.0), (5, np.inf), (3, np.nan)):  # a diagonal entry not positive and finite; an entry not finite
            bad = list(ok3)
            bad[9] = dp([v if k == e else x for k, x in enumerate(L3)])
            assert lib.rsf_dr_run(*bad) == -1, e
        assert _code(pkg, lambda: _run(eng, _state(128, 2), lo=[0.0, 0.0], hi=[1e4, 1e4])) == -1  # the solve has d = 1 or 3
        y, m = eng.dr_propose(st["q"], st["l"], *BOX1, 1.0, 1)
        assert eng.dr_ssq(y, m, np.zeros(500)).shape == (128,)
        for call in (lambda: eng.dr_ssq(y, m, np.zeros((3, 500))), lambda: eng.dr_ssq(np.ones((128, 2)), m, np.zeros(500)),
                     lambda: eng.dr_ssq(np.ones((192, 1)), np.ones(192, np.uint8), np.zeros((2, 500)))):
            assert _code(pkg, call) == -1
        assert lib.rsf_dr_ssq(ctx, 128, 1, None, P(m), P(zeros), 1, P(ones)) == -1
        assert lib.rsf_dr_ssq(ctx, 0, 1, P(y), P(m), P(zeros), 1, P(ones)) == -1
        # the Python layer refuses before any library call
        with pytest.raises(ValueError, match="stuck start"):
            eng.dr(np.full(128, 2.0e4), np.zeros(500), *BOX1, 1.0, 2)
        with pytest.raises(ValueError, match="whole workgroups"):
            eng.dr(np.full(192, 1000.0), two, *BOX1, 1.0, 2)
    # the split calls: d = 1..3, no model needed
    with pkg.Engine(mem="host", block_threads=64) as bare:
        st = _state(130, 2)
        lo, hi, L = [0.0, 0.0], [1e4, 1e4], np.array([[3.0, 0.0], [1.0, 2.0]])
        y, m = bare.dr_propose(st["q"], st["l"], lo, hi, L, 1)
        l1, pend = bare.dr_accept(st["q"], st["l"], lo, hi, 1, y, m, np.ones(130), st["c"], 250.0)
        y2, m2 = bare.dr_propose(st["q"], st["l"], lo, hi, L, 2, pending=pend)
        bare.dr_accept(st["q"], st["l"], lo, hi, 2, y2, m2, np.ones(130), st["c"], 250.0, l1=l1, pending=pend)
        for stage in (0, 3):
            assert _code(pkg, lambda: bare.dr_propose(st["q"], st["l"], lo, hi, L, stage, pending=pend)) == -1
        assert _code(pkg, lambda: bare.dr_propose(st["q"], st["l"], lo, hi, L, 2)) == -1  # stage 2 without pending
        assert bare.lib.rsf_dr_accept(bare._ctx, 130, 2, P(st["q"]), P(st["l"]), dp(lo), dp(hi), 0.2, 3, 250.0, 0, 0, 1, P(y), P(m), P(np.ascontiguousarray(y[:, 0])), P(l1), P(pend),
                                      *[P(c) for c in st["c"]]) == -1
        for kw in (dict(gamma=0.0), dict(gamma=2.0), dict(offset=-1), dict(iteration=0), dict(iteration=2 ** 32)):
            assert _code(pkg, lambda: bare.dr_propose(st["q"], st["l"], lo, hi, L, 1, **kw)) == -1, kw
            assert _code(pkg, lambda: bare.dr_accept(st["q"], st["l"], lo, hi, 1, y, m, np.ones(130), st["c"], 250.0, **kw)) == -1, kw
        assert _code(pkg, lambda: bare.dr_accept(st["q"], st["l"], lo, hi, 1, y, m, np.ones(130), st["c"], 0.0)) == -1
        assert _code(pkg, lambda: bare.dr_propose(st["q"], st["l"], lo, hi, np.stack([L, L, L]), 1)) == -1  # 130 chains over three factors
        with pytest.raises(ValueError, match="chol"):
            bare.dr_propose(st["q"], st["l"], lo, hi, np.array([[3.0, 1.0], [1.0, 2.0]]), 1)
        z4 = np.ones((130, 4))
        assert bare.lib.rsf_dr_propose(bare._ctx, 130, 4, P(z4), P(st["l"]), 1, dp([0.0] * 4), dp([2.0] * 4), dp([1.0] * 10), 0.2, 1, 0, 0, 1, None, P(z4.copy()),
                                       P(m)) == -1
        assert bare.lib.rsf_dr_propose(bare._ctx, 130, 2, None, None, 1, None, None, None, 0.2, 1, 0, 0, 1, None, None, None) == -1
        assert b"NULL" in bare.lib.rsf_last_error()


def test_error_unsupported_integrator_and_the_float32_model(pkg):
    with pkg.Engine(mem="host", block_threads=64) as eng:
        m = _model(pkg)
        m.integrator = "dop853"
        eng.set_model(m, 1)
        st = _state(128)
        assert _code(pkg, lambda: _run(eng, st)) == -5
        assert _code(pkg, lambda: eng.dr_ssq(st["q"], np.ones(128, np.uint8), np.zeros(500))) == -5
        # a float32 model gets the float64 solve: the bits of the float64 model
        data = np.cos(np.linspace(0.0, 3.0, 500))
        m = _model(pkg)
        m.precision = "float32"
        eng.set_model(m, 1)
        a = _state(128, l=-1e9)  # far below any l': the first proposals inside the box are accepted, so the solve's bits reach l
        _run(eng, a, data=data, n_iter=2, chol=[[30.0]])
        eng.set_model(_model(pkg), 1)
        b = _state(128, l=-1e9)
        _run(eng, b, data=data, n_iter=2, chol=[[30.0]])
        for k in ("q", "l"):
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)
        assert b["c"][0].sum() > 0 and (b["l"] > -1e9).any()


# ---- 8. the front ends ---------------------------------------------------------------------------------------------------------------------
def test_sample_dr_returns_a_posterior_pool(pkg, cpu_engine):
    ref, data = _reference(pkg, cpu_engine, 1, *BOX1)
    mc = pkg.MCMC(_model(pkg), data, 1000.0, ["Uniform", BOX1[0], BOX1[1]], 1000.0)
    pool = mc.sample_dr(300, 64, seed=6)  # adapt=True: the two launches of the burn-in adapt
    assert isinstance(pool, pkg.PosteriorPool) and pool.samples.shape == (32, 300, 1) and pool.std2.shape == (32, 300) and pool.nburn == 32
    s = pool.stats
    assert s["n_chains"] == 300 and s["stuck"] == 0 and s["accepted"] == s["accepted1"] + s["accepted2"] and s["chol"].shape == (1, 1, 1)
    assert s["n_solves"] == (300 * 64 - s["out_of_bounds"]) + (300 * 64 - s["accepted1"] - s["out_of_bounds2"])
    diag = pool.diagnostics()[0]
    mg = ref.marg["Dc"]
    z = (pool.samples.mean() - mg.mean) / (mg.sd / np.sqrt(diag["ess"]))
    print(f"sample_dr: accept rates {s['accept_rate1']:.3f} / {s['accept_rate2']:.3f}, Dc mean {pool.samples.mean():.2f} against {mg.mean:.2f} (sd {mg.sd:.2f}), "
          f"ESS {diag['ess']:.0f} of {32 * 300}, adapted factor {float(s['chol'][0, 0, 0]):.2f}, z {z:+.2f}")
    assert np.isfinite(pool.std2).all() and (pool.std2 > 0).all() and 0 < pool.accept_rate <= 1 and abs(z) < R.Z_MAX
    pred = pool.predictive(_model(pkg), data, max_draws=256)
    assert np.isfinite(pred["elpd_waic"]) and pred["mean"].shape == (data.size,)
    pool = mc.sample_dr(100, 8, start="fit", factor="fit", seed=6, thin=2, adapt=False)
    assert pool.samples.shape == (2, 100, 1) and pool.nburn == 4 and "fit" in pool.stats and pool.stats["stuck"] == 0
    pool = mc.sample_dr(64, 6, start=np.full((64, 1), 1000.0) + np.linspace(-50.0, 50.0, 64)[:, None], factor=[[40.0]], nburn=2, thin=2, stages=1)
    assert pool.samples.shape == (2, 64, 1) and "fit" not in pool.stats and pool.stats["accepted2"] == 0 and pool.stats["stages"] == 1


def test_inference_dr_runs_the_groups_in_one_call(pkg, cpu_engine):
    truths = (100.0, 5000.0)
    cpu_engine.set_model(_model(pkg), 1)
    data = np.stack([synthetic_data(cpu_engine, dc_true=t, seed=11 + k) for k, t in enumerate(truths)])
    problem = pkg.RSF(number_slip_values=2, lowest_slip_value=100.0, largest_slip_value=5000.0, qstart=1000.0, plotfigs=False)
    problem.model = _model(pkg)
    problem.data = data.reshape(-1)
    out = problem.inference_dr(n_chains=256, n_iter=8, nburn=4, adapt=False, seed=8, iters_per_launch=4)
    assert sorted(out) == list(truths) and problem.dr_result.chol.shape == (2, 1, 1)
    with pkg.Engine(mem="device") as dev:
        dev.set_model(_model(pkg), 1)
        for g, dc in enumerate(truths):
            pool = out[dc]
            one = dev.dr(np.full((256, 1), 1000.0), data[g], *BOX1, problem.dr_result.chol[g], 8, seed=8, offset=256 * g, keep=4, iters_per_launch=4)
            print(f"inference_dr Dc_true {dc}: accept rates {pool.stats['accept_rate1']:.3f} / {pool.stats['accept_rate2']:.3f}, Dc mean {pool.samples.mean():.2f}")
            np.testing.assert_array_equal(pool.samples, one.trace_q)
            assert pool.samples.shape == (4, 256, 1) and pool.std2.shape == (4, 256) and pool.stats["n_solves"] == one.n_solves
            assert len(pool.diagnostics()) == 1
