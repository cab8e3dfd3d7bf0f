"""
GPU tests of the multi-start Levenberg-Marquardt fit (include/rsf_fit.h: rsf_fit_normal / _run / _trial / _decide / _laplace;
Engine.fit, Engine.fit_from_residuals, MCMC.fit, RSF.inference_fit) against the specification tests/fit_reference.py.

1. rsf_fit_normal against the extended-precision RK4 (tests/rk4_extended.forward_ext through init_extended's X): ssq to rtol 1e-9
   (tier 1); jtj over sqrt(H_pp H_rr) and grad over sqrt(H_pp ssq) within twice the distance of the float64 specification fed with
   the checker's solve from the same reference, plus that specification's own median as a floor (the ratio form of
   test_gpu_rk4_extended.py, on the maximum and on the median of a case's starts).
2. the split path on closed forms against the specification, decision for decision.
3. the fused kernel against the split path on the real model, the first four iterations.
4., 5. Engine.fit at d = 1 and d = 3 against the specification on the checker.
6. contracts.
Every test prints what it measured before it asserts.
"""
import numpy as np
import pytest

import fit_reference as F
import init_extended as I
import rk4_extended as X
from test_fit_reference import STARTS, checker_problem

pytestmark = pytest.mark.gpu

LD = np.longdouble
LO1, HI1 = [0.0], [1.0e4]
LO3, HI3 = [0.0, 1e-3, 1e-3], [1.0e4, 0.1, 0.1]
STARTS3 = ((1000.0, 0.011, 0.014), (3000.0, 0.02, 0.03), (300.0, 0.005, 0.02))
_CACHE = {}


def _model(pkg, nsteps=500, substeps=1):
    m = pkg.RateStateModel(number_time_steps=nsteps)
    m.RadiationDamping = True
    m.substeps = substeps
    return m


def _checker_solve(eng, d):
    if d == 1:
        return lambda pts: np.asarray(eng.forward(np.ascontiguousarray(pts[:, 0]))[1])
    return lambda pts: np.asarray(eng.forward(*(np.ascontiguousarray(pts[:, p]) for p in range(3)))[1])


def _ext_solve(m, d):
    if d == 1:
        return lambda pts: X.forward_ext(m, pts[:, 0])[0]
    return lambda pts: X.forward_ext(m, pts[:, 0], pts[:, 1], pts[:, 2])[0]


# ---- 1. the normal equations against extended precision ---------------------------------------------------------------------------
#          name: (nsteps, substeps, d, n, observation rows, workgroup threads)
NORMAL_CASES = {
    "d1_n3": (500, 1, 1, 3, 1, 0),
    "d1_n33_wave_edge": (500, 1, 1, 33, 1, 0),      # 32 pairs fill a wave: start 32 is the first of the second
    "d3_n17_wave_edge": (500, 1, 3, 17, 1, 0),      # 16 quads fill a wave
    "d1_n133_partial_workgroup": (500, 1, 1, 133, 1, 0),  # 128 pairs fill a workgroup of 256
    "d1_two_rows": (500, 1, 1, 128, 2, 64),         # two observation series, 64 starts each: workgroups of 64 threads, 32 starts
    "d3_two_rows": (500, 1, 3, 128, 2, 64),
    "d1_substeps2": (500, 2, 1, 3, 1, 0),
    "d1_two_chunks": (800, 4, 1, 3, 1, 0),          # kc = 796 < nout - 1 (test_gpu_smc_batch.py, test_chunked_table)
}


def _normal_errors(got, ref):
    ssq, g, H = (np.asarray(x, dtype=np.float64) for x in got)
    rs, rg, rH = ref
    sd = np.sqrt(np.diagonal(rH, axis1=1, axis2=2))
    e_s = (np.abs(I._w(ssq) - rs) / rs).astype(np.float64)
    e_h = (np.abs(I._w(H) - rH) / (sd[:, :, None] * sd[:, None, :])).max(axis=(1, 2)).astype(np.float64)
    e_g = (np.abs(I._w(g) - rg) / (sd * np.sqrt(rs)[:, None])).max(axis=1).astype(np.float64)
    return e_s, e_g, e_h


@pytest.mark.parametrize("name", list(NORMAL_CASES))
def test_normal_equations_against_extended_precision(pkg, cpu_engine, name):
    nsteps, S, d, n, G, block = NORMAL_CASES[name]
    m = _model(pkg, nsteps, S)
    fd = 1e-6 if d == 1 else 1e-4
    rng = np.random.default_rng(7)
    q = np.linspace(300.0, 3000.0, n)[:, None]
    if d == 3:
        q = np.concatenate([q, 0.011 + 0.004 * rng.random((n, 1)), 0.014 + 0.004 * rng.random((n, 1))], axis=1)
    truth = X.forward_ext(m, np.array([1000.0, 400.0][:G]))[0].astype(np.float64).T
    data = truth + 0.01 * np.abs(truth).max() * rng.standard_normal(truth.shape)
    np.testing.assert_array_equal(F.perturbed(q, fd), I.perturbed_points(m, q, fd)[:, :, :d])  # init_extended's points, and its X below
    ref = F.normal(_ext_solve(m, d), q, data, fd, out=LD)
    cpu_engine.set_model(m, S)
    o = _normal_errors(F.normal(_checker_solve(cpu_engine, d), q, data, fd), ref)
    with pkg.Engine(mem="host", block_threads=block) as eng:
        assert eng.set_model(m, S) == data.shape[1]
        got = eng.fit_normal(q, data if G > 1 else data[0], fd)
        g = _normal_errors(got, ref)
        if G == 1 and d == 1:  # the sum of squares rsf_mcmc_init computes, to rounding (that kernel fuses the sample's product into the residual)
            eng.mcmc_init(q, data[0], LO1, HI1, n0=0.0)
            np.testing.assert_allclose(got[0], eng.get_state()[1], rtol=1e-13, atol=0)
    fails = []
    print(f"{name}: ssq gpu max {g[0].max():.2e} | specification max {o[0].max():.2e}")
    for what, ge, oe in (("grad", g[1], o[1]), ("jtj", g[2], o[2])):
        floor = np.median(oe)
        print(f"{name} {what}: gpu max {ge.max():.2e} med {np.median(ge):.2e} | specification max {oe.max():.2e} med {floor:.2e} | "
              f"ratio max {ge.max() / oe.max():.2f} med {np.median(ge) / floor:.2f}")
        if not (ge.max() <= 2 * oe.max() + floor and np.median(ge) <= 2 * floor + floor):
            fails.append(what)
    assert g[0].max() <= 1e-9
    assert not fails, fails
    assert np.array_equal(got[2], np.swapaxes(got[2], 1, 2))  # jtj is stored full and symmetric


# ---- 2. the split path on closed forms, decision for decision ----------------------------------------------------------------------
def _state_arrays(st):
    return [st[k] for k in ("q", "ssq", "g", "H", "lam", "status", "iters")]


def _compare_split(eng, normal_fn, q0, lo, hi, ftol, n_iter, tag, first=None):
    """n_iter iterations of the specification and of rsf_fit_trial / rsf_fit_decide side by side -> the two final states.  Both are
    fed with normal_fn at the SPECIFICATION's trial points: the GPU's lie within 1e-13 of the box width of them (asserted), but a
    forward difference of step 1e-6 would turn that into 1e-9 of grad and jtj, and the two chains would drift apart by more than
    the rounding this test is about.  The GPU's q is its own throughout."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    q0 = np.asarray(q0, dtype=np.float64)
    st = F.new_state(q0, *(normal_fn(q0) if first is None else first))
    gs = {k: v.copy() for k, v in st.items()}
    margin = np.inf
    for it in range(n_iter):
        before = st["ssq"].copy()
        run = st["status"] == F.RUNNING
        qt, ok = F.trials(st, lo, hi)
        s_n, g_n, h_n = normal_fn(qt)
        acc = F.decide(st, qt, ok, s_n, g_n, h_n, ftol)
        dec = run & ok & np.isfinite(s_n)
        if dec.any():  # no decision of the specification may be a near tie
            margin = min(margin, float((np.abs(s_n[dec] - before[dec]) / before[dec]).min()))
        gqt, gok = eng.fit_trial(gs["q"], gs["g"], gs["H"], gs["lam"], gs["status"], lo, hi)
        np.testing.assert_array_equal(gok.astype(bool), ok, err_msg=f"{tag} iteration {it}: ok")
        e = float((np.abs(gqt - qt) / (hi - lo)).max())
        assert e <= 1e-13, (tag, it, e)
        gs_n, gg_n, gh_n = s_n, g_n, h_n
        lam_before = gs["lam"].copy()
        eng.fit_decide(gs["q"], gs["ssq"], gs["g"], gs["H"], gs["lam"], gs["status"], gs["iters"], gqt, gok, gs_n, gg_n, gh_n, ftol)
        np.testing.assert_array_equal(run & (gs["lam"] <= lam_before), acc, err_msg=f"{tag} iteration {it}: accept")  # a rejection raises lam
        np.testing.assert_array_equal(gs["status"], st["status"], err_msg=f"{tag} iteration {it}: status")
        np.testing.assert_array_equal(gs["iters"], st["iters"], err_msg=f"{tag} iteration {it}: iters")
        np.testing.assert_array_equal(gs["lam"], st["lam"], err_msg=f"{tag} iteration {it}: lam")
        assert float((np.abs(gs["q"] - st["q"]) / (hi - lo)).max()) <= 1e-13, (tag, it)
    print(f"{tag}: {n_iter} iterations, starts per status {np.bincount(st['status'], minlength=4).tolist()}, most iterations {int(st['iters'].max())}, "
          f"smallest |ssq' - ssq| / ssq at a decision {margin:.2e}")
    assert margin > 1e-9, (tag, margin)
    return st, gs


def test_split_path_on_closed_forms(pkg, gpu_engine):
    eng = gpu_engine
    t = np.linspace(0.0, 5.0, 60)
    rng = np.random.default_rng(12)

    def decay(pts):
        return np.exp(-t[:, None] / pts[None, :, 0]) * np.sin(3.0 * t)[:, None] + 0.1 * np.log1p(pts[None, :, 0])

    def curve3(pts):
        return np.exp(-t[:, None] / pts[None, :, 0]) + pts[None, :, 1] * t[:, None] + pts[None, :, 2]

    def amp2(pts):
        return pts[None, :, 0] * np.exp(-t[:, None] / pts[None, :, 1])

    # d = 1: accepted and rejected steps, 257 starts (a second workgroup of the split kernels).  ftol 1e-2 ends a start while its
    # decreases are still far above the rounding noise, and the iteration counts stop before any start reaches it: the smallest
    # |ssq' - ssq| / ssq at a decision is 2e-6 here, 2e-5 and 7e-5 in the two cases below (asserted > 1e-9 in _compare_split)
    data = decay(np.array([[4.0]]))[:, 0] + 0.02 * rng.standard_normal(t.size)
    q0 = np.concatenate([[0.3, 0.5, 2.0, 9.0, 30.0, 49.0], np.linspace(0.6, 45.0, 251)])[:, None]
    st, _ = _compare_split(eng, lambda p: F.normal(decay, p, data, 1e-6), q0, [0.1], [50.0], 1e-2, 5, "decay d=1")
    assert (st["status"] == F.CONVERGED).sum() >= 20 and (st["lam"] > F.LAM0).any()  # some rejections happened
    # the same data in a box that ends before the minimum: the first step is clamped one ulp inside the edge
    st, gs = _compare_split(eng, lambda p: F.normal(decay, p, data, 1e-6), [[2.0], [2.5]], [0.1], [3.0], 1e-2, 1, "decay d=1, edge")
    assert (gs["q"] == np.nextafter(3.0, 0.0)).all()
    # d = 2 and d = 3
    data = amp2(np.array([[1.5, 2.0]]))[:, 0] + 0.01 * rng.standard_normal(t.size)
    _compare_split(eng, lambda p: F.normal(amp2, p, data, 1e-6), [[0.5, 0.7], [3.0, 5.0], [1.0, 1.0]], [0.0, 0.1], [10.0, 10.0], 1e-2, 4, "amplitude d=2")
    data = curve3(np.array([[3.0, 0.02, 0.5]]))[:, 0] + 1e-3 * rng.standard_normal(t.size)
    q0 = [[2.0, 0.01, 0.3], [5.0, 0.05, 1.0], [1.0, -0.2, 2.0], [20.0, 0.3, -1.0]]
    _compare_split(eng, lambda p: F.normal(curve3, p, data, 1e-4), q0, [0.1, -1.0, -5.0], [50.0, 1.0, 5.0], 1e-4, 4, "curve d=3")
    # crafted states: a factor that fails sixteen times (STALLED at lam > 1e12), a first sum that is not finite (FAILED, unmoved), a
    # trial whose sum is not finite (rejected), next to an ordinary accepted step
    first = (np.array([2.0, np.nan, 2.0, 2.0]), np.full((4, 1), 1.0), np.array([0.0, 1.0, 1.0, 1.0]).reshape(4, 1, 1))
    # (the last start's sum falls by a tenth per step of 1e-3: accepted every time, lam down to its floor of 1e-12 and staying there)
    fn = lambda p: (np.array([1.0, 1.0, np.inf, np.exp(100.0 * (p[3, 0] - 5.0))]), np.full((4, 1), 1e-3), np.ones((4, 1, 1)))
    st, gs = _compare_split(eng, fn, np.full((4, 1), 5.0), [0.0], [10.0], 1e-4, 17, "crafted", first=first)
    assert st["status"].tolist() == [F.STALLED, F.FAILED, F.STALLED, F.RUNNING] and st["iters"].tolist() == [16, 0, 16, 17]
    assert gs["q"][1, 0] == 5.0 and gs["q"][0, 0] == 5.0 and np.isnan(gs["ssq"][1])


# ---- the real model at nsteps 500 -------------------------------------------------------------------------------------------------
def _real(pkg, cpu_engine, dc_true):
    if dc_true not in _CACHE:
        _CACHE[dc_true] = checker_problem(pkg, cpu_engine, dc_true)[0]
    return _CACHE[dc_true]


def _grid_min(eng, data, dc_true):
    grid = np.linspace(0.98 * dc_true, 1.02 * dc_true, 4001)
    return float(np.asarray(eng.forward(grid, data=data, want_ssq=True, want_acc=False)[0]).min())


def _gpu_state(pkg, eng, q0, data, fd):
    ssq, g, H = eng.fit_normal(q0, data, fd)
    n = q0.shape[0]
    return {"q": q0.copy(), "ssq": ssq, "g": g, "H": H, "lam": np.full(n, pkg._abi.FIT_LAM0),
            "status": np.where(np.isfinite(ssq), pkg._abi.FIT_RUNNING, pkg._abi.FIT_FAILED).astype(np.int32), "iters": np.zeros(n, dtype=np.int32)}


def _run(eng, st, data, lo, hi, fd, ftol, n_iter):
    eng.fit_run(st["q"], data, lo, hi, st["ssq"], st["g"], st["H"], st["lam"], st["status"], st["iters"], n_iter, fd, ftol)


def _bits(st):
    return [np.ascontiguousarray(x).view(np.uint8 if x.dtype.itemsize == 1 else (np.int32 if x.dtype.itemsize == 4 else np.int64)) for x in _state_arrays(st)]


# ---- 3. fused against split ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_fused_against_split_on_the_real_model(pkg, gpu_engine, cpu_engine, d):
    data = _real(pkg, cpu_engine, 1000.0)
    eng = gpu_engine
    eng.set_model(_model(pkg), 1)
    q0 = np.array(STARTS)[:, None] if d == 1 else np.array(STARTS3)
    lo, hi, fd = (LO1, HI1, 1e-6) if d == 1 else (LO3, HI3, 1e-4)
    fused = _gpu_state(pkg, eng, q0, data, fd)
    split = {k: v.copy() for k, v in fused.items()}
    identical = True
    for it in range(4):
        _run(eng, fused, data, lo, hi, fd, F.FTOL, 1)
        qt, ok = eng.fit_trial(split["q"], split["g"], split["H"], split["lam"], split["status"], lo, hi)
        s_n, g_n, h_n = eng.fit_normal(qt, data, fd)
        eng.fit_decide(split["q"], split["ssq"], split["g"], split["H"], split["lam"], split["status"], split["iters"], qt, ok, s_n, g_n, h_n, F.FTOL)
        same = all(np.array_equal(a, b) for a, b in zip(_bits(fused), _bits(split)))
        identical = identical and same
        print(f"d {d} iteration {it}: lam {fused['lam'].tolist()} status {fused['status'].tolist()} bit-identical {same}, "
              f"ssq relative difference {float(np.abs(fused['ssq'] / split['ssq'] - 1).max()):.2e}")
        # the same accept decisions: lam, status and iters carry them
        for k in ("lam", "status", "iters"):
            np.testing.assert_array_equal(fused[k], split[k], err_msg=f"iteration {it}: {k}")
        np.testing.assert_allclose(fused["ssq"], split["ssq"], rtol=1e-9, atol=0)
    # four iterations inside one launch: the bits of four launches of one
    once = _gpu_state(pkg, eng, q0, data, fd)
    _run(eng, once, data, lo, hi, fd, F.FTOL, 4)
    for a, b in zip(_bits(once), _bits(fused)):
        np.testing.assert_array_equal(a, b)
    # measured on the MI355X: the fused kernel and the split path (rsf_fit_normal's kernel at the trial points) give the same
    # bits at every one of the four iterations, d = 1 and 3 — asserted instead of the tolerance above, which it implies
    print(f"d {d}: fused and split paths bit-identical over the four iterations: {identical}")
    assert identical


# ---- 4. Engine.fit, d = 1 -----------------------------------------------------------------------------------------------------------
def _fit_d1(pkg, cpu_engine):
    """the problem of items 4 and 6: two groups (Dc_true 100 and 5000), the five starts each -> (data (2, nout), q0 (10, 1), the
    specification's fit on the checker, one state per group)"""
    if "d1" not in _CACHE:
        truths = (100.0, 5000.0)
        data = np.stack([_real(pkg, cpu_engine, t) for t in truths])
        cpu_engine.set_model(_model(pkg), 1)
        solve = _checker_solve(cpu_engine, 1)
        spec = [F.fit(lambda p, g=g: F.normal(solve, p, data[g], 1e-6), np.array(STARTS)[:, None], LO1, HI1) for g in range(2)]
        _CACHE["d1"] = (truths, data, np.tile(np.array(STARTS), 2)[:, None], spec)
    return _CACHE["d1"]


def test_engine_fit_one_parameter(pkg, gpu_engine, cpu_engine):
    truths, data, q0, spec = _fit_d1(pkg, cpu_engine)
    eng = gpu_engine
    eng.set_model(_model(pkg), 1)
    res = eng.fit(q0, data, LO1, HI1, max_iter=60)
    for g, t in enumerate(truths):
        sl = slice(5 * g, 5 * g + 5)
        gmin = _grid_min(eng, data[g], t)
        dq = np.abs(res.q[sl, 0] / spec[g]["q"][:, 0] - 1)
        print(f"Dc_true {t}: status {res.status[sl].tolist()} iters {res.iters[sl].tolist()} (specification {spec[g]['status'].tolist()} "
              f"{spec[g]['iters'].tolist()}), ssq / grid minimum - 1 {(res.ssq[sl] / gmin - 1).tolist()}, q against the specification {dq.tolist()}")
        assert (res.status[sl] == pkg._abi.FIT_CONVERGED).all() and (res.iters[sl] <= 60).all()
        assert (res.ssq[sl] <= (1 + 1e-9) * gmin).all()
        assert dq.max() <= 1e-7
        i = res.best(g)
        lap = res.laplace(None, LO1, HI1, i)
        print(f"Dc_true {t}: best {res.q[i, 0]!r} +- {lap['stderr'][0]:.3e}, Laplace log evidence {lap['log_evidence']!r}")
        assert sl.start <= i < sl.stop and abs(res.q[i, 0] - t) <= 6 * lap["stderr"][0]


# ---- 5. Engine.fit, d = 3 -----------------------------------------------------------------------------------------------------------
def test_engine_fit_three_parameters(pkg, gpu_engine, cpu_engine):
    data = _real(pkg, cpu_engine, 1000.0)
    q0 = np.array(STARTS3)[1:2]
    cpu_engine.set_model(_model(pkg), 1)
    spec = F.fit(lambda p: F.normal(_checker_solve(cpu_engine, 3), p, data, 1e-4), q0, LO3, HI3, max_iter=60)
    eng = gpu_engine
    eng.set_model(_model(pkg), 1)
    res = eng.fit(q0, data, LO3, HI3, max_iter=60)
    gmin = _grid_min(eng, data, 1000.0)
    prod, want = res.q[0, 0] * res.q[0, 1], spec["q"][0, 0] * spec["q"][0, 1]
    print(f"d 3: status {res.status.tolist()} iters {res.iters.tolist()} q {res.q[0].tolist()} (specification {spec['q'][0].tolist()}), "
          f"ssq / d = 1 grid minimum - 1 {res.ssq[0] / gmin - 1!r} (specification {spec['ssq'][0] / gmin - 1!r}), Dc a {prod!r} against {want!r}: {abs(prod / want - 1):.2e}")
    assert res.iters[0] <= 60 and res.ssq[0] < gmin
    assert abs(prod / want - 1) <= 1e-3


# ---- 6. contracts -------------------------------------------------------------------------------------------------------------------
def test_host_and_device_memory_give_the_same_bits(pkg, gpu_engine, cpu_engine):
    _, data, q0, _ = _fit_d1(pkg, cpu_engine)
    gpu_engine.set_model(_model(pkg), 1)
    host = gpu_engine.fit(q0, data, LO1, HI1, max_iter=16)
    with pkg.Engine(mem="device") as dev:
        dev.set_model(_model(pkg), 1)
        got = dev.fit(q0, data, LO1, HI1, max_iter=16)
    for k in ("q", "ssq", "grad", "jtj", "lam", "status", "iters"):
        np.testing.assert_array_equal(getattr(got, k), getattr(host, k), err_msg=k)


def test_finished_and_failed_starts_are_not_written(pkg, gpu_engine, cpu_engine):
    data = _real(pkg, cpu_engine, 1000.0)
    eng = gpu_engine
    eng.set_model(_model(pkg), 1)
    # 0.05 is stiff: fixed-step RK4 gives a sum that is not finite (test_gpu_parity.py) — FAILED, and it stays where it is
    q0 = np.array([0.05, 30.0, 300.0, 1000.0, 3000.0, 9000.0])[:, None]
    st = _gpu_state(pkg, eng, q0, data, 1e-6)
    assert not np.isfinite(st["ssq"][0]) and st["status"].tolist() == [pkg._abi.FIT_FAILED] + [pkg._abi.FIT_RUNNING] * 5
    _run(eng, st, data, LO1, HI1, 1e-6, F.FTOL, 10)
    done = st["status"] != pkg._abi.FIT_RUNNING
    print(f"after 10 iterations: status {st['status'].tolist()} iters {st['iters'].tolist()}")
    assert done[0] and st["q"][0, 0] == 0.05 and st["iters"][0] == 0 and st["lam"][0] == pkg._abi.FIT_LAM0
    assert 1 < done.sum() < 6  # some starts have finished, some are still running
    before = _bits({k: v.copy() for k, v in st.items()})
    _run(eng, st, data, LO1, HI1, 1e-6, F.FTOL, 3)
    for a, b in zip(before, _bits(st)):
        np.testing.assert_array_equal(a[done], b[done])
    assert (st["iters"][~done] > 10).all()
    res = eng.fit(q0, data, LO1, HI1)
    assert res.status[0] == pkg._abi.FIT_FAILED and res.q[0, 0] == 0.05 and res.best() != 0


def test_error_codes(pkg, gpu_engine):
    eng = gpu_engine
    q, data = np.array([[1000.0], [2000.0]]), np.zeros(500)
    with pytest.raises(pkg.RsfError, match="set_model") as ei:
        eng.fit_normal(q, data)
    assert ei.value.code == -3
    eng.set_model(_model(pkg), 1)
    ssq, g, H = eng.fit_normal(q, data)
    st = {"q": q.copy(), "ssq": ssq, "g": g, "H": H, "lam": np.full(2, 1e-3), "status": np.zeros(2, dtype=np.int32), "iters": np.zeros(2, dtype=np.int32)}

    def code(call):
        with pytest.raises(pkg.RsfError) as ei:
            call()
        return ei.value.code

    assert code(lambda: eng.fit_normal(np.zeros((2, 2)), data)) == -1                      # d = 2 has no solve
    assert code(lambda: eng.fit_normal(q, data, 0.0)) == -1
    assert code(lambda: eng.fit_normal(np.zeros((6, 1)) + 1000.0, np.zeros((2, 500)))) == -1  # 3 starts per series: not whole workgroups
    assert code(lambda: _run(eng, st, data, LO1, HI1, 1e-6, 1e-9, 0)) == -1
    assert code(lambda: _run(eng, st, data, LO1, HI1, 1e-6, 1e-9, 65)) == -1
    assert code(lambda: _run(eng, st, data, LO1, HI1, 1e-6, -1.0, 1)) == -1
    assert code(lambda: _run(eng, st, data, [5.0], [5.0], 1e-6, 1e-9, 1)) == -1
    assert code(lambda: eng.fit_trial(np.zeros((2, 4)), np.zeros((2, 4)), np.zeros((2, 4, 4)), st["lam"], st["status"], [0.0] * 4, [1.0] * 4)) == -1
    assert code(lambda: eng.fit_trial(st["q"], st["g"], st["H"], st["lam"], st["status"], [0.0], [np.inf])) == -1
    assert code(lambda: eng.fit_decide(st["q"], st["ssq"], st["g"], st["H"], st["lam"], st["status"], st["iters"], st["q"], np.zeros(2, dtype=np.uint8),
                                       st["ssq"], st["g"], st["H"], np.nan)) == -1
    assert eng.lib.rsf_fit_normal(eng._ctx, 2, 1, None, None, 1, 1e-6, None, None, None) == -1 and b"NULL" in eng.lib.rsf_last_error()
    # the reference's integrator has no fit; a float32 model gets the float64 solve
    m = _model(pkg)
    m.integrator = "dop853"
    eng.set_model(m, 1)
    assert code(lambda: eng.fit_normal(q, data)) == -5
    assert code(lambda: _run(eng, st, data, LO1, HI1, 1e-6, 1e-9, 1)) == -5
    m = _model(pkg)
    m.precision = "float32"
    eng.set_model(m, 1)
    np.testing.assert_allclose(eng.fit_normal(q, data)[0], ssq, rtol=1e-12, atol=0)


def test_front_ends_return_the_group_optima(pkg, gpu_engine, cpu_engine):
    truths, data, q0, _ = _fit_d1(pkg, cpu_engine)
    gpu_engine.set_model(_model(pkg), 1)
    res = gpu_engine.fit(q0, data, LO1, HI1, max_iter=60)
    best = [res.q[res.best(g), 0] for g in range(2)]
    for g, t in enumerate(truths):
        mc = pkg.MCMC(_model(pkg), data[g], t, ["Uniform", 0.0, 1.0e4], 1000.0)
        r = mc.fit(n_starts=8, seed=1, max_iter=60)
        assert r.q.shape == (8, 1) and r.q[0, 0] != 1000.0 and r.n_groups == 1
        print(f"MCMC.fit Dc_true {t}: best {r.q[r.best(), 0]!r} against {best[g]!r}, statuses {r.status.tolist()}")
        assert abs(r.q[r.best(), 0] / best[g] - 1) <= 1e-7
    problem = pkg.RSF(number_slip_values=2, lowest_slip_value=100.0, largest_slip_value=5000.0, qstart=1000.0, plotfigs=False)
    problem.model = _model(pkg)
    problem.data = data.reshape(-1)
    out = problem.inference_fit(n_starts=8, seed=1, max_iter=60)
    assert sorted(out) == [100.0, 5000.0] and problem.fit_result.q.shape == (16, 1)
    for g, t in enumerate(truths):
        print(f"RSF.inference_fit Dc_true {t}: {out[t]}")
        assert abs(out[t]["q"][0] / best[g] - 1) <= 1e-7 and out[t]["stderr"].shape == (1,) and 8 * g <= out[t]["index"] < 8 * g + 8
    # fit_from_residuals on the GPU: the split kernels under the Python loop, on a closed form
    t_ = np.linspace(0.0, 5.0, 40)
    obs = np.exp(-t_ / 3.0) + 1e-3 * np.sin(7.0 * t_)
    r = gpu_engine.fit_from_residuals(lambda p: np.exp(-t_[None, :] / p[:, :1]) - obs[None, :], [1.0, 8.0], 0.1, 50.0)
    print(f"fit_from_residuals: q {r.q[:, 0].tolist()} status {r.status.tolist()} iters {r.iters.tolist()}")
    assert np.abs(r.q[:, 0] - 3.0).max() <= 0.05 and abs(r.q[0, 0] / r.q[1, 0] - 1) <= 1e-7 and (r.status != pkg._abi.FIT_RUNNING).all()
