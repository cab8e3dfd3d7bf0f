"""
GPU tests of the Levenberg-Marquardt fit under either state law and any observable (include/rsf_law_fit.h: rsf_law_fit_normal /
rsf_law_fit_run; Engine.law_fit_normal / law_fit_run / law_fit; MCMC.fit_law; RSF.inference_law):
  1. the normal equations: ssq is rsf_law_observe's bit for bit, grad and jtj are fit_reference.normal's on the GPU's own series;
  2. a start's neighbours do not matter;
  3. the fused kernel against the split path rsf_fit_trial -> rsf_law_fit_normal -> rsf_fit_decide, bit for bit;
  4. two groups are two one-group calls;
  5. the default model agrees with the ageing fit's tiers;
  6. Engine.law_fit at d = 1 and 7. at d = 3 against the specification (tests/law_fit_reference.py);
  8. the front ends;  9. the error codes through ctypes.
The common problem is tests/test_gpu_law_dr.py's: nsteps 500 under the step history, truth (Dc, a, b) = (20, 0.011, 0.014), noise 5 %
of the excursion (observe_reference.bf_data); boxes (5, 200) at d = 1 and (8, 0.009, 0.012) .. (60, 0.013, 0.016) at d = 3.
"""
import functools

import numpy as np
import pytest

import fit_reference as F
import law_cases as C
import law_fit_reference as LF
import law_reference as R
import observe_cases as OC
import observe_reference as O

pytestmark = pytest.mark.gpu

LD = np.longdouble
FIELDS = ("q", "ssq", "grad", "jtj", "lam", "status", "iters")
FAIL_DC = 0.05  # no trajectory of either law is finite there, at 1 or 8 substeps (the specification's too)


def _model(pkg, nsteps=500, substeps=1, history="step", **attrs):
    m = pkg.RateStateModel(number_time_steps=nsteps)
    m.substeps = substeps
    if history == "step":
        m.loading = R.step_history
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _bits(x):
    x = np.ascontiguousarray(np.asarray(x.cpu() if hasattr(x, "cpu") else x))
    return x.view(np.int32 if x.dtype.itemsize == 4 else (np.uint8 if x.dtype.itemsize == 1 else np.int64))


@functools.lru_cache(maxsize=None)
def _series(law, history="step", dc=R.BF_TRUTH, substeps=1):
    """all four clean series of the specification at Dc = dc, from one solve"""
    m = C.spec(500, substeps)
    return {k: v[:, 0] for k, v in O.trajectory(m, [dc], R.table(m, history), law).items()}


@functools.lru_cache(maxsize=None)
def _data(law, obs, history="step", dc=R.BF_TRUTH, substeps=1, draw=0):
    """bf_data's recipe: the clean series plus 5 % of its excursion (of its size for the acceleration) N(0, 1), default_rng(BF_SEED + draw)"""
    clean = _series(law, history, dc, substeps)[obs]
    return clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(R.BF_SEED + draw).standard_normal(clean.size)


def _points(d, n, seed=0):
    lo, hi = LF.BOX[d]
    return np.ascontiguousarray(lo + (hi - lo) * np.random.default_rng([n, d, seed]).uniform(0.05, 0.95, (n, d)))


def _starts(d, n):
    rng = np.random.default_rng(7)
    return np.ascontiguousarray(np.column_stack([rng.uniform(15.0, 25.0, n), rng.uniform(0.0105, 0.0115, n), rng.uniform(0.0135, 0.0145, n)])[:, :d])


def _observe(eng, law, obs, pts, data=None):
    """law_observe at points (m, d) -> (ssq or None, series (nout, m)) on the host"""
    ab = [np.ascontiguousarray(pts[:, p]) for p in (1, 2)] if pts.shape[1] == 3 else [None, None]
    ssq, s = eng.law_observe(law, obs, np.ascontiguousarray(pts[:, 0]), ab[0], ab[1], data=data, want_ssq=data is not None, want_series=True)
    return ssq, np.asarray(s)


def _new_state(eng, q, normal):
    """the state Engine.law_fit builds from the first normal equations, in the engine's memory space"""
    ssq, grad, jtj = normal
    host = np.asarray(ssq.cpu() if hasattr(ssq, "cpu") else ssq)
    n = len(host)
    return dict(q=eng._in(np.array(q, dtype=np.float64)), ssq=ssq, grad=grad, jtj=jtj, lam=eng._in(np.full(n, F.LAM0)),
                status=eng._ints(np.where(np.isfinite(host), F.RUNNING, F.FAILED)), iters=eng._ints(np.zeros(n)))


def _copy(st):
    return {k: (v.clone() if hasattr(v, "clone") else v.copy()) for k, v in st.items()}


def _run(eng, law, obs, st, data, lo, hi, n_iter, fd, ftol):
    eng.law_fit_run(law, obs, st["q"], data, lo, hi, st["ssq"], st["grad"], st["jtj"], st["lam"], st["status"], st["iters"], n_iter, fd, ftol)


# ---- 1. the normal equations ---------------------------------------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("obs", O.OBSERVABLES)
@pytest.mark.parametrize("law", R.LAWS)
def test_normal_equations(pkg, law, obs):
    """ssq: law_observe's bits.  grad and jtj against fit_reference.normal on the GPU's own law_observe series of the (d + 1) n points,
    summed in long double: |got - want| over sum_k |X_pk| (|s_k| + |data_k|) (grad) or sum_k |X_pk X_rk| (jtj) is at most
    (nout + 8) 2^-53 — a recursive fma sum of nout terms, three roundings in X (the difference, the reciprocal, the product), and for
    the acceleration the fma residual against the rounded sample.  Measured on an MI355X, the largest over the eight cases: grad 2.33e-15
    (ageing, acc), jtj 4.19e-15 (slip, theta), against the bound 5.64e-14."""
    worst = {"grad": 0.0, "jtj": 0.0}
    with pkg.Engine(mem="host") as eng:
        B = eng.block_threads
        for history in ("builtin", "step"):
            data = _data(law, obs, history)
            for damping in (True, False):
                eng.set_model(_model(pkg, history=history, RadiationDamping=damping), 1)
                bound = (eng.nout + 8) * 2.0 ** -53
                for d in (1, 3):
                    fd = LF.FD[d]
                    for n in (1, 17, B // (d + 1) + 1):
                        q = _points(d, n)
                        ssq, grad, jtj = (np.asarray(x) for x in eng.law_fit_normal(law, obs, q, data))
                        tag = (law, obs, history, damping, d, n)
                        want_ssq, _ = _observe(eng, law, obs, q, data)
                        assert np.isfinite(ssq).all() and np.array_equal(_bits(ssq), _bits(want_ssq)), tag
                        flat = _observe(eng, law, obs, np.ascontiguousarray(F.perturbed(q, fd).reshape(-1, d)))[1]  # the (d + 1) n trajectories, once
                        _, g, H = F.normal(lambda pts: flat, q, data, fd, out=LD)
                        s = flat.reshape(-1, d + 1, n).astype(LD)
                        X = np.stack([np.abs(s[:, p + 1] - s[:, 0]) / (np.abs(F.perturbed(q, fd)[p + 1, :, p]) * fd) for p in range(d)])  # (d, nout, n)
                        sg = np.stack([(X[p] * (np.abs(s[:, 0]) + np.abs(data)[:, None])).sum(axis=0) for p in range(d)], axis=1)
                        sH = np.stack([np.stack([(X[p] * X[r]).sum(axis=0) for r in range(d)], axis=1) for p in range(d)], axis=1)
                        eg, eH = float((np.abs(grad - g) / sg).max()), float((np.abs(jtj - H) / sH).max())
                        worst["grad"], worst["jtj"] = max(worst["grad"], eg), max(worst["jtj"], eH)
                        assert eg <= bound and eH <= bound, (tag, eg, eH, bound)
                        assert np.array_equal(jtj, jtj.transpose(0, 2, 1)), tag  # full and symmetric
    WORST[law, obs] = worst
    print(f"{law} {obs}: largest |got - want| / scale: grad {worst['grad']:.2e}, jtj {worst['jtj']:.2e}; the bound {bound:.2e}; "
          f"so far over all cases: grad {max(w['grad'] for w in WORST.values()):.2e} jtj {max(w['jtj'] for w in WORST.values()):.2e}")


# ---- 2. neighbours do not matter -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_neighbours_do_not_matter(pkg, d):
    law, obs, fd, ftol = "slip", "mu", LF.FD[d], 1e-9
    data = _data(law, obs)
    lo, hi = LF.BOX[d]
    star = np.array([17.3, 0.0108, 0.0141])[:d]
    crowd = _starts(d, 256)
    crowd[100] = star
    crowd[99, 0], crowd[101, 0] = C.LOW  # the slip law's trajectory is not finite there
    model = _model(pkg)
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        alone = _new_state(eng, star[None], eng.law_fit_normal(law, obs, star[None], data))
        among = _new_state(eng, crowd, eng.law_fit_normal(law, obs, crowd, data))
        assert not np.isfinite(among["ssq"][[99, 101]]).any() and np.isfinite(np.delete(among["ssq"], [99, 101])).all()
        assert among["status"][[99, 101]].tolist() == [F.FAILED, F.FAILED] and among["status"].sum() == 2 * F.FAILED
        first = _copy(among)
        for k in ("ssq", "grad", "jtj"):
            assert np.array_equal(_bits(alone[k][0]), _bits(among[k][100])), k
        _run(eng, law, obs, alone, data, lo, hi, 3, fd, ftol)
        _run(eng, law, obs, among, data, lo, hi, 3, fd, ftol)
        for k in FIELDS:
            assert np.array_equal(_bits(alone[k][0]), _bits(among[k][100])), k
            assert np.array_equal(_bits(first[k][[99, 101]]), _bits(among[k][[99, 101]])), k  # a FAILED start is never written
        assert alone["iters"][0] >= 1 and not np.array_equal(alone["q"][0], star)
        # the driver: FIT_FAILED for a first SSq that is not finite, and such a start keeps its point
        res = eng.law_fit(law, obs, crowd, data, lo, hi, max_iter=3, iters_per_launch=3)
        assert res.status[[99, 101]].tolist() == [F.FAILED, F.FAILED] and np.array_equal(res.q[[99, 101]], crowd[[99, 101]]) and res.best() not in (99, 101)
        for k in FIELDS:
            assert np.array_equal(_bits(getattr(res, k)), _bits(among[k])), k
    # device memory: the same bits
    import torch

    with pkg.Engine(mem="device") as dev:
        dev.set_model(model, 1)
        st = _new_state(dev, crowd, dev.law_fit_normal(law, obs, dev._in(crowd), data))
        _run(dev, law, obs, st, data, lo, hi, 3, fd, ftol)
        torch.cuda.synchronize()
        for k in FIELDS:
            assert np.array_equal(_bits(st[k]), _bits(among[k])), f"device memory: {k}"


# ---- 3. fused against split ------------------------------------------------------------------------------------------------------------------
# The box ends BELOW the optimum (Dc <= 19.5; the data's truth is 20) and ftol is 1e-3, so that four iterations hold every branch, as
# the specification run on these starts shows (tests/law_fit_reference.py, the first four cases: accepted / of trial points per
# iteration 101 65 0 0 / 101 100 100 100; 50 43 7 22 / 65 65 64 64; 64 62 64 50 / 65 65 65 52; 101 85 54 23 / 101 98 95 92): every
# start walks up to the clamp at nextafter(19.5, lo), accepted; from there the trial point is the same point again, ssq' == ssq, a
# rejection; a start a hair below the edge is CONVERGED by its first accepted step; the starts of the second wave sit at FAIL_DC,
# FAILED from the first normal equations on, so that wave has no RUNNING start while the others of its workgroup solve.
FUSED_CASES = {
    "ageing, mu, d1": dict(law="aging", obs="mu", d=1, n=133),
    "slip, acc, d3": dict(law="slip", obs="acc", d=3, n=81),
    "slip, mu, d3, undamped": dict(law="slip", obs="mu", d=3, n=81, damping=False),
    "ageing, acc, d1": dict(law="aging", obs="acc", d=1, n=133),
    "slip, mu, d1, two chunks": dict(law="slip", obs="mu", d=1, n=133, substeps=8),
}
FUSED_HI = 19.5


def _fused_starts(d, n, per):
    rng = np.random.default_rng(11)
    q = np.column_stack([rng.uniform(8.5, 19.4, n), rng.uniform(0.0105, 0.0115, n), rng.uniform(0.0135, 0.0145, n)])
    q[per:2 * per, 0] = FAIL_DC
    q[0] = [19.49, 0.011, 0.014]
    q[1:4, 0] = [19.4999, 19.49999, 19.499999]
    return np.ascontiguousarray(q[:, :d])


@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_fused_against_split(pkg, name):
    c = FUSED_CASES[name]
    law, obs, d, n, sub = c["law"], c["obs"], c["d"], c["n"], c.get("substeps", 1)
    fd, ftol = LF.FD[d], 1e-3
    data = _data(law, obs, substeps=sub)
    lo, hi = LF.BOX[d][0].copy(), LF.BOX[d][1].copy()
    hi[0] = FUSED_HI
    model = _model(pkg, 500, sub, RadiationDamping=c.get("damping", True))
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, sub)
        # the table and the observation in one chunk of the staging budget, or in two (the chunk size: the engine's, as test_gpu_law_dr.py takes it)
        assert (2 * sub * (eng.nout - 1) + 1 + eng.nout > 56 * 1024 // 8) == (sub == 8)
        per = 64 // (d + 1)  # the starts of one wave
        assert eng.block_threads == 256 and n * (d + 1) > eng.block_threads
        q0 = _fused_starts(d, n, per)
        fused = _new_state(eng, q0, eng.law_fit_normal(law, obs, q0, data))
        wave = slice(per, 2 * per)
        assert (fused["status"][wave] == F.FAILED).all() and (np.delete(fused["status"], np.arange(per, 2 * per)) == F.RUNNING).all()
        split, once, first = _copy(fused), _copy(fused), _copy(fused)
        seen = dict(accepted=0, rejected=0, clamped=0)
        for it in range(1, 5):
            _run(eng, law, obs, fused, data, lo, hi, 1, fd, ftol)
            before = _copy(split)
            qt, ok = eng.fit_trial(split["q"], split["grad"], split["jtj"], split["lam"], split["status"], lo, hi)
            assert not ok[wave].any()
            ssq_n, g_n, H_n = eng.law_fit_normal(law, obs, qt, data, fd)
            eng.fit_decide(split["q"], split["ssq"], split["grad"], split["jtj"], split["lam"], split["status"], split["iters"], qt, ok, ssq_n, g_n, H_n, ftol)
            same = {k: bool(np.array_equal(_bits(fused[k]), _bits(split[k]))) for k in FIELDS}
            run = before["status"] == F.RUNNING
            acc, rej = run & (split["lam"] < before["lam"]), run & (split["lam"] > before["lam"])
            clamp = (ok != 0)[:, None] & ((qt == np.nextafter(lo, hi)) | (qt == np.nextafter(hi, lo)))
            seen["accepted"] += int(acc.sum()); seen["rejected"] += int(rej.sum()); seen["clamped"] += int(clamp.sum())
            print(f"{name} iteration {it}: running {int(run.sum())} trial points {int(ok.sum())} accepted {int(acc.sum())} rejected {int(rej.sum())} clamped "
                  f"coordinates {int(clamp.sum())} statuses {np.bincount(split['status'], minlength=4).tolist()}; bit-identical {same}")
            assert all(same.values()), same
            assert (acc | rej).sum() == run.sum() and np.array_equal(split["iters"], before["iters"] + run)
        assert seen["accepted"] > 0 and seen["rejected"] > 0 and seen["clamped"] > 0, seen
        assert (fused["status"] == F.CONVERGED).any() and (fused["status"][wave] == F.FAILED).all()
        for k in FIELDS:  # a FAILED start is never written
            assert np.array_equal(_bits(fused[k][wave]), _bits(first[k][wave])), k
        # four iterations inside one launch: the bits of four launches of one
        _run(eng, law, obs, once, data, lo, hi, 4, fd, ftol)
        for k in FIELDS:
            np.testing.assert_array_equal(_bits(once[k]), _bits(fused[k]), err_msg=k)


# ---- 4. groups ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_two_groups_are_two_calls(pkg, d):
    law, obs = "slip", "mu"
    two = np.stack([_data(law, obs), _data(law, obs, draw=1)])
    lo, hi = LF.BOX[d]
    per = 40  # not a whole workgroup of 64 threads: each series' starts are padded with 24 copies of its first start
    q0 = _starts(d, 2 * per)
    with pkg.Engine(mem="host", block_threads=64) as eng:
        eng.set_model(_model(pkg), 1)
        both = eng.law_fit(law, obs, q0, two, lo, hi, max_iter=12, iters_per_launch=4)
        assert both.n_groups == 2 and both.q.shape == (2 * per, d) and per <= both.best(1) < 2 * per
        for g in range(2):
            sl = slice(g * per, (g + 1) * per)
            one = eng.law_fit(law, obs, q0[sl], two[g], lo, hi, max_iter=12, iters_per_launch=4)
            for k in FIELDS:
                np.testing.assert_array_equal(_bits(getattr(both, k)[sl]), _bits(getattr(one, k)), err_msg=f"group {g}: {k}")
            assert (one.status != F.FAILED).all() and (one.iters > 0).all()
        # the normal equations alone, whole workgroups per series
        q = _points(d, 128)
        got = eng.law_fit_normal(law, obs, q, two)
        for g in range(2):
            want = eng.law_fit_normal(law, obs, q[g * 64:(g + 1) * 64], two[g])
            for a, b in zip(got, want):
                np.testing.assert_array_equal(_bits(a[g * 64:(g + 1) * 64]), _bits(b))


# ---- 5. the default model agrees with the ageing fit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_default_model_agrees_with_the_ageing_fit(pkg, d):
    model = pkg.RateStateModel(number_time_steps=500)
    rng = np.random.default_rng(3)
    q = np.column_stack([rng.uniform(200.0, 3000.0, 65), rng.uniform(0.0105, 0.0115, 65), rng.uniform(0.0135, 0.0145, 65)])[:, :d]
    q = np.ascontiguousarray(q)
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        acc = np.asarray(eng.forward([1000.0])[1])[:, 0]
        data = acc + np.abs(acc) * np.random.default_rng(2025).standard_normal(acc.size)
        tier = eng.fit_normal(q, data)[0]
        plain = eng.law_fit_normal("aging", "acc", q, data)[0]
    err = np.abs(plain / tier - 1).max()
    print(f"d {d}: largest |law_fit_normal's ssq / fit_normal's - 1| {err:.2e}")
    assert np.isfinite(plain).all() and err <= C.CAP


# ---- 6. Engine.law_fit, d = 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("truth", R.LAWS)
def test_engine_law_fit_one_parameter(pkg, truth):
    """test_gpu_fit.py's bounds for the same algorithm: ssq within 1 + 1e-9 of the specification's best, q within 1e-7 of the
    specification's start by start; the best Dc within one posterior SD of the quadrature's mean (the specification meets all three and
    ends CONVERGED: tests/test_law_fit_reference.py)."""
    p, spec = OC.friction_problem(truth), LF.fit_d1(truth)
    model = _model(pkg, observable="mu", state_law=truth)
    model.loading = p["vl"]
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        res = eng.law_fit(truth, "mu", np.array(LF.STARTS1)[:, None], p["data"], *LF.BOX[1], max_iter=60)
    best = spec["ssq"].min()
    dq = np.abs(res.q[:, 0] / spec["q"][:, 0] - 1)
    i = res.best()
    print(f"truth {truth}: status {res.status.tolist()} iters {res.iters.tolist()} (specification {spec['status'].tolist()} {spec['iters'].tolist()}), "
          f"ssq / specification's best - 1 {(res.ssq / best - 1).tolist()}, q against the specification {dq.tolist()}; best Dc {res.q[i, 0]!r}, "
          f"quadrature mean {p['mean'][truth]!r} sd {p['sd'][truth]!r}")
    assert (res.status == F.CONVERGED).all() and (res.iters <= 60).all()
    assert (res.ssq <= (1 + 1e-9) * best).all()
    assert dq.max() <= 1e-7
    assert abs(res.q[i, 0] - p["mean"][truth]) <= p["sd"][truth]


# ---- 7. Engine.law_fit, d = 3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("truth", R.LAWS)
def test_engine_law_fit_three_parameters(pkg, truth):
    """test_engine_fit_three_parameters' tolerances: the best start's ssq below the one-parameter minimum, its product Dc a within 1e-3
    of the specification's, and here its ssq too.  LF.STARTS3 as first chosen: the specification converges from all four."""
    p, spec, spec1 = OC.friction_problem(truth), LF.fit_d3(truth), LF.fit_d1(truth)
    model = _model(pkg, observable="mu", state_law=truth)
    model.loading = p["vl"]
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        res = eng.law_fit(truth, "mu", np.array(LF.STARTS3), p["data"], *LF.BOX[3], max_iter=60)
    i, j = res.best(), int(np.argmin(spec["ssq"]))
    prod, want = res.q[i, 0] * res.q[i, 1], spec["q"][j, 0] * spec["q"][j, 1]
    print(f"truth {truth}: status {res.status.tolist()} iters {res.iters.tolist()} q {res.q[i].tolist()} (specification {spec['q'][j].tolist()}), ssq "
          f"{res.ssq[i]!r} against {spec['ssq'][j]!r}: {abs(res.ssq[i] / spec['ssq'][j] - 1):.2e}; Dc a {prod!r} against {want!r}: {abs(prod / want - 1):.2e}")
    assert (res.iters <= 60).all() and res.ssq[i] < spec1["ssq"].min()
    assert abs(res.ssq[i] / spec["ssq"][j] - 1) <= 1e-3 and abs(prod / want - 1) <= 1e-3


# ---- 8. the front ends -----------------------------------------------------------------------------------------------------------------------------
def test_fit_law_returns_the_specifications_best_point(pkg):
    p = OC.friction_problem("slip")
    model = _model(pkg, observable="mu", state_law="slip")
    model.loading = p["vl"]
    mc = pkg.MCMC(model, p["data"], R.BF_TRUTH, ["Uniform", *R.BF_BOX], 40.0, nsamples=10, verbose=False)
    r = mc.fit_law(n_starts=8, seed=1, max_iter=60)
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        q0, lo, hi = mc._fit_starts(eng, 8, 1)
    spec = LF.fit(p["m"], p["vl"], "slip", "mu", q0, p["data"], lo, hi, LF.FD[1], max_iter=60)
    got, want = r.q[r.best(), 0], spec["q"][int(np.argmin(spec["ssq"])), 0]
    print(f"MCMC.fit_law: best {got!r} against the specification's {want!r}, statuses {r.status.tolist()} (specification {spec['status'].tolist()})")
    assert r.q.shape == (8, 1) and q0[0, 0] == 40.0 and r.n_groups == 1 and (spec["status"] == F.CONVERGED).all()
    assert abs(got / want - 1) <= 1e-7
    # the methods of the ageing-only kernels still refuse this model, by name
    with pytest.raises(NotImplementedError, match="fit integrates the ageing law only"):
        mc.fit()
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        with pytest.raises(NotImplementedError, match="this call integrates the ageing law only"):
            eng.fit(q0, p["data"], lo, hi)
        eng.set_model(_model(pkg, observable="mu"), 1)
        with pytest.raises(NotImplementedError, match="this call fits the acceleration only"):
            eng.fit(q0, p["data"], lo, hi)


def test_fit_law_on_the_default_model_is_fit(pkg):
    model = pkg.RateStateModel(number_time_steps=500)
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        acc = np.asarray(eng.forward([1000.0])[1])[:, 0]
    data = acc + np.abs(acc) * np.random.default_rng(2025).standard_normal(acc.size)
    mc = pkg.MCMC(model, data, 1000.0, ["Uniform", 0.0, 1.0e4], 1000.0, nsamples=10, verbose=False)
    a, b = mc.fit(n_starts=8, seed=1, max_iter=60), mc.fit_law(n_starts=8, seed=1, max_iter=60)
    print(f"default model: MCMC.fit best {a.q[a.best(), 0]!r} (statuses {a.status.tolist()}), MCMC.fit_law best {b.q[b.best(), 0]!r} (statuses {b.status.tolist()})")
    assert abs(b.q[b.best(), 0] / a.q[a.best(), 0] - 1) <= 1e-7


def test_inference_law(pkg):
    law, truths = "slip", (20.0, 30.0)
    problem = pkg.RSF(number_slip_values=2, lowest_slip_value=truths[0], largest_slip_value=truths[1], qstart=40.0, qpriors=["Uniform", *R.BF_BOX], plotfigs=False)
    problem.model = _model(pkg, observable="mu", state_law=law)
    problem.data = np.concatenate([_data(law, "mu", dc=t) for t in truths])
    fits, pools = problem.inference_law(n_chains=64, n_iter=64, nburn=0, n_starts=8, seed=1, max_iter=60)
    assert sorted(fits) == sorted(pools) == list(truths) and problem.fit_result.q.shape == (16, 1) and problem.fit_result.n_groups == 2
    for g, t in enumerate(truths):
        f, pool = fits[t], pools[t]
        x = np.asarray(pool.samples)
        print(f"RSF.inference_law Dc_true {t}: fit {f['q'].tolist()} +- {f['stderr'].tolist()} status {f['status']}; pooled mean {x.mean():.4f} SD {x.std():.4f}, "
              f"accept rate {pool.accept_rate:.2f}")
        assert sorted(f) == ["cov", "index", "iters", "q", "ssq", "status", "stderr"] and 8 * g <= f["index"] < 8 * g + 8 and f["status"] == F.CONVERGED
        assert abs(f["q"][0] - t) <= 6 * f["stderr"][0]
        assert pool.stats["path"] == "law_dr" and x.shape == (64, 64, 1) and np.isfinite(x).all() and np.isfinite(np.asarray(pool.std2)).all()
        # the chains start at the fit's point: a chain whose first iteration rejected both stages is still there, and no chain is far from it
        assert (x[0, :, 0] == f["q"][0]).any() and np.abs(x[0, :, 0] - f["q"][0]).max() <= 20 * f["stderr"][0]


# ---- 9. the error codes through ctypes ---------------------------------------------------------------------------------------------------------
def _plain(pkg, **attrs):
    m = pkg.RateStateModel(number_time_steps=500)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_error_codes(pkg):
    P = lambda x: x.ctypes.data
    dp = lambda v: np.atleast_1d(np.asarray(v, dtype=np.float64)).ctypes.data_as(pkg._abi._DP)
    n = 128
    q, zeros, two = np.ascontiguousarray(np.linspace(900.0, 1100.0, n)[:, None]), np.zeros(500), np.zeros((2, 500))
    ssq, grad, jtj, lam = np.ones(n), np.zeros((n, 1)), np.ones((n, 1, 1)), np.full(n, 1e-3)
    status, iters = np.zeros(n, np.int32), np.zeros(n, np.int32)
    with pkg.Engine(mem="host", block_threads=64) as eng:
        lib, ctx = eng.lib, eng._ctx
        normal = lambda law=1, obs=1: [ctx, law, obs, n, 1, P(q), P(zeros), 1, 1e-6, P(ssq), P(grad), P(jtj)]
        run = lambda law=1, obs=1: [ctx, law, obs, n, 1, P(q), P(zeros), 1, dp(0.0), dp(1e4), 1e-6, 1e-9, 1, P(ssq), P(grad), P(jtj), P(lam), P(status), P(iters)]
        calls = (("rsf_law_fit_normal", lib.rsf_law_fit_normal, normal), ("rsf_law_fit_run", lib.rsf_law_fit_run, run))
        # no model: RSF_ERR_STATE
        for name, fn, args in calls:
            assert fn(*args()) == -3 and name.encode() in lib.rsf_last_error()
        eng.set_model(_plain(pkg), 1)
        for name, fn, args in calls:
            assert fn(*args()) == 0, name
        # the law and the observable: rsf_law_observe's messages
        for name, fn, args in calls:
            for law in (-1, 2, 7):
                assert fn(*args(law=law)) == -1 and (name + ": law is RSF_LAW_AGEING").encode() in lib.rsf_last_error()
            for obs in (-1, 4):
                assert fn(*args(obs=obs)) == -1 and (name + ": observable is RSF_OBS_ACC").encode() in lib.rsf_last_error()
        # every argument error of rsf_fit_normal and rsf_fit_run, under this function's name (the arguments lie two places further on)
        bad_normal = ((3, 0), (4, 2), (4, 4), (5, None), (6, None), (7, 0), (8, 0.0), (8, np.nan), (8, np.inf), (9, None), (10, None), (11, None))
        bad_run = ((3, 0), (4, 2), (5, None), (6, None), (7, 0), (8, None), (9, None), (8, dp(np.nan)), (9, dp(np.inf)), (10, 0.0), (10, np.nan), (11, -1.0),
                   (11, np.inf), (12, 0), (12, 65), (13, None), (14, None), (15, None), (16, None), (17, None), (18, None))
        for (name, fn, args), bads in zip(calls, (bad_normal, bad_run)):
            for i, v in bads:
                bad = args()
                bad[i] = v
                assert fn(*bad) == -1, (name, i)
                assert name.encode() in lib.rsf_last_error(), (name, i)
            assert fn(None, *args()[1:]) == -1 and name.encode() in lib.rsf_last_error()
        bad = run()
        bad[8], bad[9] = dp(5.0), dp(5.0)
        assert lib.rsf_law_fit_run(*bad) == -1
        # groups in whole workgroups of 64 threads: 2 x 64 starts pass, 2 x 48 do not
        grp = lambda m: [ctx, 1, 1, m, 1, P(q), P(two), 2, 1e-6, P(ssq), P(grad), P(jtj)]
        assert lib.rsf_law_fit_normal(*grp(96)) == -1 and b"rsf_law_fit_normal" in lib.rsf_last_error() and lib.rsf_law_fit_normal(*grp(128)) == 0
        # the integrator: RSF_ERR_UNSUPPORTED
        eng.set_model(_plain(pkg, integrator="dop853"), 1)
        for name, fn, args in calls:
            assert fn(*args()) == -5 and name.encode() in lib.rsf_last_error()
        # a float32-flagged default model gets the float64 solve: the bits of the float64 model
        data = np.cos(np.linspace(0.0, 3.0, 500))
        out = []
        for attrs in (dict(precision="float32"), dict()):
            eng.set_model(_plain(pkg, **attrs), 1)
            st = _new_state(eng, q, eng.law_fit_normal("aging", "acc", q, data))
            _run(eng, "aging", "acc", st, data, [0.0], [1e4], 2, 1e-6, 1e-9)
            out.append(st)
        for k in FIELDS:
            np.testing.assert_array_equal(_bits(out[0][k]), _bits(out[1][k]), err_msg=k)
        assert (out[1]["iters"] == 2).all()
