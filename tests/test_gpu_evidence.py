"""
GPU tests of the marginal likelihood by bridge sampling (include/rsf_evidence.h: rsf_evidence_propose / _logg / _logtarget /
_partials / _finish; Engine.evidence*, bayes_factor) against the long double specification tests/evidence_reference.py.

Bounds (tests/evidence_cases.py, where the measurements and the reasoning are recorded): theta 8 x 9.1e-16 relative, log g
8 x 5.6e-14 over max(|log g|, 1), the partials' sums 8 x 3.5e-16 relative, the converged log_integral 2 TOL_PARTIAL + 7.1e-15;
the fused kernel's l within shape x 1e-9 of the specification fed with the checker's SSq (tier 1's rtol on SSq through the
logarithm); the end-to-end estimates within Z_MAX = 4.5 of the SPECIFICATION's re on the same draws.
"""
import ctypes

import numpy as np
import pytest

import evidence_cases as cases
import evidence_reference as ref
import posterior_reference as R
import psis_cases
from conftest import synthetic_data

pytestmark = pytest.mark.gpu

LD = np.longdouble
_CACHE = {}


def _normals(eng, seed, offset, n, d):
    return np.array([eng.draws(seed, offset + j, 0, d, 12.0)[0] for j in range(n)]).reshape(n, d)


# ---- 1. the proposal -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [p[0] for p in cases.PROPOSALS])
def test_proposal(gpu_engine, name):
    (mean, chol, tr, lo, hi), = [p[1:] for p in cases.PROPOSALS if p[0] == name]
    d, seed, nmax = len(mean), 11, max(cases.N2S)
    z = _CACHE.setdefault(("z", d), _normals(gpu_engine, seed, cases.OFFSET, nmax, d))
    want_t, want_g, _ = ref.propose(z, mean, chol, tr, lo, hi, LD)
    full = None
    for n2 in cases.N2S:
        theta, logg, inb = gpu_engine.evidence_propose(mean, chol, lo, hi, n2, tr, seed=seed, offset=cases.OFFSET)
        et = float(np.abs((theta - want_t[:n2]) / want_t[:n2]).max())
        eg = float((np.abs(logg - want_g[:n2]) / np.maximum(np.abs(want_g[:n2]), 1)).max())
        print(f"{name} n2 {n2}: theta {et:.3e} (relative), logg {eg:.3e} (scaled), {int(inb.sum())} inside the box")
        assert et <= cases.TOL_THETA and eg <= cases.TOL_LOGG
        np.testing.assert_array_equal(inb.astype(bool), ref.inbox(theta, lo, hi))
        full = (theta, logg, inb)
    theta, logg, inb = full
    assert 0 < inb.sum() < nmax  # both sides of the box occur
    # the same density code for given points
    g = gpu_engine.evidence_logg(theta, mean, chol, tr)
    wg = ref.logg(theta, mean, chol, tr, LD)
    assert float((np.abs(g - wg) / np.maximum(np.abs(wg), 1)).max()) <= cases.TOL_LOGG
    # points exactly on lo and on hi are outside: the box moved onto two of the draws
    lo2, hi2 = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    idx = np.flatnonzero(inb)
    i, j = idx[np.argmin(theta[idx, 0])], idx[np.argmax(theta[idx, d - 1])]
    lo2[0], hi2[d - 1] = theta[i, 0], theta[j, d - 1]
    t2, _, inb2 = gpu_engine.evidence_propose(mean, chol, lo2, hi2, nmax, tr, seed=seed, offset=cases.OFFSET)
    np.testing.assert_array_equal(t2, theta)
    np.testing.assert_array_equal(inb2.astype(bool), ref.inbox(theta, lo2, hi2))
    assert not inb2[i] and not inb2[j] and inb2.sum() == inb.sum() - 2
    # two shards with offsets 0 and k are one call of k + m
    k = 300
    a = gpu_engine.evidence_propose(mean, chol, lo, hi, k, tr, seed=seed, offset=cases.OFFSET)
    b = gpu_engine.evidence_propose(mean, chol, lo, hi, nmax - k, tr, seed=seed, offset=cases.OFFSET + k)
    for x, y, w in zip(a, b, full):
        np.testing.assert_array_equal(np.concatenate([x, y]), w)


# ---- 2. the bridge reduction ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", cases.BRIDGE_SIZES)
def test_bridge_reduction(pkg, gpu_engine, n1, n2):
    l1, l2, lstar = cases.crafted_l(n1, n2)
    for r in (1.0, 0.37):
        got, want = gpu_engine.evidence_partials(l1, l2, lstar, r), ref.partials(l1, l2, lstar, r, dtype=LD).astype(np.float64)
        np.testing.assert_array_equal(got[:3], want[:3])
        nz = want[3:] != 0
        e = float(np.abs((got[3:][nz] - want[3:][nz]) / want[3:][nz]).max())
        print(f"({n1}, {n2}) r {r}: partials {e:.3e} (relative)")
        assert e <= cases.TOL_PARTIAL and (got[3:][~nz] == 0).all()
        assert np.isfinite(got).all()
    res, wres = gpu_engine.evidence_bridge(l1, l2, lstar=lstar), ref.bridge(l1, l2, lstar=lstar, dtype=LD)
    print(f"({n1}, {n2}): log_integral {res['log_integral']!r} against {float(wres['log_integral'])!r}, {res['iterations']} iterations")
    assert res["converged"] and wres["converged"] and res["iterations"] == wres["iterations"]
    assert abs(res["log_integral"] - float(wres["log_integral"])) <= cases.TOL_LOGI
    assert res["n2_in_box"] == wres["n2_in_box"] == int(np.isfinite(l2).sum()) and res["log_evidence"] is None
    if min(n1, n2) >= 2:
        assert res["re"] == pytest.approx(float(wres["re"]), rel=1e-9)
    else:
        assert res["re"] == np.inf
    # three uneven shards with the pool's s1, s2 against one call
    s1, s2 = n1 / (n1 + n2), n2 / (n1 + n2)
    parts = sum(gpu_engine.evidence_partials(l1[a], l2[b], lstar, 0.37, s1, s2) for a, b in zip(cases.shards(n1), cases.shards(n2)))
    np.testing.assert_allclose(parts, got, rtol=1e-12, atol=0)
    # host and device memory: the same bits
    with pkg.Engine(mem="device") as dev:
        np.testing.assert_array_equal(dev.evidence_partials(l1, l2, lstar, 0.37), got)
        np.testing.assert_array_equal(gpu_engine.evidence_partials(l1, l2, lstar, 0.37), got)


@pytest.mark.parametrize("n1,n2", cases.BRIDGE_SIZES_CAPPED)
def test_bridge_partials_past_the_grid_cap(pkg, gpu_engine, n1, n2):
    """evidence_terms_kernel where its grid-stride loop takes a second and a third trip, at the bound of test_bridge_reduction."""
    l1, l2, lstar = cases.crafted_l(n1, n2)
    left_out = int(np.isneginf(l2).sum())
    assert left_out > n2 // 20
    for r in (1.0, 0.37):
        got, want = gpu_engine.evidence_partials(l1, l2, lstar, r), ref.partials(l1, l2, lstar, r, dtype=LD).astype(np.float64)
        np.testing.assert_array_equal(got[:3], want[:3])
        assert got[0] == n1 and got[1] == n2 and got[2] == n2 - left_out
        nz = want[3:] != 0
        e = float(np.abs((got[3:][nz] - want[3:][nz]) / want[3:][nz]).max())
        print(f"({n1}, {n2}) r {r}: partials {e:.3e} (relative), {left_out} proposal draws left out")
        assert nz.all() and e <= cases.TOL_PARTIAL and np.isfinite(got).all()
    with pkg.Engine(mem="device") as dev:
        np.testing.assert_array_equal(dev.evidence_partials(l1, l2, lstar, 0.37), got)


def test_bridge_without_a_draw_in_the_support(gpu_engine):
    l1, _, lstar = cases.crafted_l(1037, 5)
    res = gpu_engine.evidence_bridge(l1, np.full(257, -np.inf), lstar=lstar, shape=12.0, lo=[0.0], hi=[1.3])
    assert res["log_integral"] == -np.inf and res["log_evidence"] == -np.inf and res["re"] == np.inf
    assert res["converged"] is False and res["n2_in_box"] == 0 and res["iterations"] == 1
    part = gpu_engine.evidence_partials(l1, np.full(257, -np.inf), lstar, 1.0)
    assert not np.isnan(part).any() and part[3] == 0 and gpu_engine.evidence_finish(part, 1.0, lstar)["r_next"] == 0.0
    # either set may be empty
    assert gpu_engine.evidence_partials(l1, [], lstar, 1.0, 0.5, 0.5)[1] == 0
    assert gpu_engine.evidence_partials([], [0.0, -np.inf], lstar, 1.0, 0.5, 0.5)[0] == 0


# ---- 3. the fused kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("d,n", [(1, 63), (1, 1037), (3, 63), (3, 1037)])
def test_fused_logtarget(pkg, gpu_engine, cpu_engine, d, n, damping):
    model, q, _, data = psis_cases.real_draws(pkg, cpu_engine, n, d, 700 + d + n)
    model.RadiationDamping = damping
    cpu_engine.set_model(model, 1)
    gpu_engine.set_model(model, 1)
    lo, hi = np.array([0.0, 0.009, 0.013])[:d], np.array([1600.0, 0.013, 0.017])[:d]
    q[3, 0] = 1700.0   # outside the box
    q[7, 0] = 0.0      # on the edge: outside the strict box
    q[11, 0] = 0.2     # inside the box, stiff: the fixed-step series is not finite
    if d == 3:
        q[13, 2] = 0.0175
    tr = np.array([0, 1, 0][:d] if d == 3 else [0], dtype=np.int32)
    shape = 0.5 * data.size
    logg = np.random.default_rng(n).uniform(-12.0, -3.0, n)
    ssq, _ = cpu_engine.forward(q[:, 0], a=q[:, 1] if d == 3 else None, b=q[:, 2] if d == 3 else None, data=data, want_ssq=True, want_acc=False)
    want = ref.logtarget(q, ssq, shape, lo, hi, tr, logg, LD).astype(np.float64)
    got = gpu_engine.evidence_logtarget(q, data, lo, hi, logg, transform=tr)
    out = np.isneginf(want)
    np.testing.assert_array_equal(np.isneginf(got), out)
    assert out[[3, 7, 11]].all() and (d == 1 or out[13]) and out.sum() == (3 if d == 1 else 4) and not np.isnan(got).any()
    e = float(np.abs(got[~out] - want[~out]).max())
    print(f"d {d} n {n} damping {damping}: l within {e:.3e} (bound {shape * 1e-9:.3e})")
    assert e <= shape * 1e-9
    # a wave wholly outside the box: -inf throughout, and the next wave's values unchanged
    q2 = q.copy()
    if n > 64:
        q2[:64, 0] = 1700.0
        g2 = gpu_engine.evidence_logtarget(q2, data, lo, hi, logg, transform=tr)
        assert np.isneginf(g2[:64]).all()
        np.testing.assert_array_equal(g2[64:], got[64:])


# ---- 4. end to end, the closed forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_end_to_end_closed_form(gpu_engine, d):
    post, fn, c = R.closed_reference(d)
    ssq_fn = lambda q: fn(*np.asarray(q).reshape(-1, d).T)
    N = cases.CLOSED_N
    q = post.draw(np.random.default_rng(40 + d), 2 * N)
    res = gpu_engine.evidence_from_ssq(q, ssq_fn, c["lo"], c["hi"], c["shape"], seed=3)
    # the specification on the same draws: the library's proposal draws are the normals of (seed 3, chain j, iteration 0)
    theta, _, _ = gpu_engine.evidence_propose(res["mean"], res["chol"], c["lo"], c["hi"], N, seed=3)
    z = np.linalg.solve(res["chol"], (theta - res["mean"]).T).T
    want = ref.evidence(q, ssq_fn, c["lo"], c["hi"], c["shape"], z)
    err = res["log_integral"] - cases.CLOSED_TRUTH[d]
    print(f"d = {d}: log I^ {res['log_integral']:.8f}, error {err:+.2e}, re {res['re']:.3e} (specification {float(want['re']):.3e}), "
          f"{res['iterations']} iterations, {res['n2_in_box']} of {N} inside the box")
    assert res["converged"] and res["n1"] == res["n2"] == N and res["ess_factor"] == 1.0
    assert float(want["re"]) <= cases.CLOSED_RE_MAX
    assert abs(err) < R.Z_MAX * float(want["re"])
    assert res["re"] == pytest.approx(float(want["re"]), rel=1e-9)
    vol = np.log(np.asarray(c["hi"]) - np.asarray(c["lo"])).sum()
    from math import lgamma

    assert res["log_evidence"] == pytest.approx(res["log_integral"] - vol + lgamma(c["shape"]) - c["shape"] * np.log(np.pi), abs=1e-12)
    assert res["shape"] == c["shape"] and res["n_data"] == 24


# ---- 5. end to end, the real model ------------------------------------------------------------------------------------------
def test_end_to_end_real_model(pkg, gpu_engine, cpu_engine):
    model = pkg.RateStateModel(number_time_steps=500)
    model.RadiationDamping = True
    cpu_engine.set_model(model, 1)
    data = synthetic_data(cpu_engine)
    shape, lo, hi = 0.5 * data.size, 0.0, 1.0e4
    fn = R.checker_ssq(cpu_engine, data)
    post, fine = R.Posterior1(fn, lo, hi, shape, n_fine=4001), R.Posterior1(fn, lo, hi, shape, n_fine=8001)
    truth, truth_fine = np.log(post.Z) + post.lmax, np.log(fine.Z) + fine.lmax
    N = cases.CLOSED_N
    q = post.draw(np.random.default_rng(77), 2 * N)
    gpu_engine.set_model(model, 1)
    res = gpu_engine.evidence(q, data, lo, hi, seed=5)
    theta, _, _ = gpu_engine.evidence_propose(res["mean"], res["chol"], [lo], [hi], N, seed=5)
    z = (theta - res["mean"]) / res["chol"][0, 0]
    want = ref.evidence(q, lambda x: fn(np.asarray(x).reshape(-1)), [lo], [hi], shape, z)
    unc = post.outside + abs(truth_fine - truth)
    err = res["log_integral"] - truth
    print(f"real model d = 1: log I^ {res['log_integral']:.6f}, truth {truth:.6f} (n_fine 8001: {truth_fine:.6f}, outside {post.outside:.1e}), "
          f"error {err:+.2e}, re {res['re']:.3e} (specification {float(want['re']):.3e}), {res['n2_in_box']} of {N} inside the box")
    assert unc < float(want["re"]) / 10
    assert res["converged"] and res["shape"] == shape and res["n_data"] == data.size
    assert abs(err) < R.Z_MAX * float(want["re"])


def test_kept_trace_takes_its_ess_from_the_diagnostics(gpu_engine):
    """A kept trace (n, C, d) of independent draws: the factor comes from diagnostics' ESS of f2 and is near 1; a flat pool has 1."""
    post, fn, c = R.closed_reference(1)
    q = post.draw(np.random.default_rng(9), 256 * 64).reshape(256, 64, 1)
    ssq_fn = lambda x: fn(*np.asarray(x).reshape(-1, 1).T)
    tr = gpu_engine.evidence_from_ssq(q, ssq_fn, c["lo"], c["hi"], c["shape"])
    flat = gpu_engine.evidence_from_ssq(q.reshape(-1, 1), ssq_fn, c["lo"], c["hi"], c["shape"])
    assert flat["ess_factor"] == 1.0 and 0.5 < tr["ess_factor"] <= 1.0
    assert tr["log_integral"] == flat["log_integral"] and tr["re"] >= flat["re"]
    assert tr["n1"] == 128 * 64


# ---- 6. bayes_factor ---------------------------------------------------------------------------------------------------------
def test_bayes_factor(pkg, gpu_engine):
    post, fn, c = R.closed_reference(1)
    q = post.draw(np.random.default_rng(2), 4096)
    ssq_fn = lambda x: fn(*np.asarray(x).reshape(-1, 1).T)
    a = gpu_engine.evidence_from_ssq(q, ssq_fn, c["lo"], c["hi"], c["shape"])
    # a box twice as wide, downwards, where SSq^-shape is below 5^-12 of its peak: the same integral, half the prior density
    b = gpu_engine.evidence_from_ssq(q, ssq_fn, [-1.3], c["hi"], c["shape"], seed=1)
    bf = pkg.bayes_factor(a, b)
    assert bf["re"] == pytest.approx(np.hypot(a["re"], b["re"]))
    assert abs(bf["log_bf"] - np.log(2.0)) < R.Z_MAX * bf["re"] + 1e-6
    other = gpu_engine.evidence_from_ssq(q, ssq_fn, c["lo"], c["hi"], 12.5)
    with pytest.raises(ValueError):
        pkg.bayes_factor(a, other)
    with pytest.raises(ValueError):
        pkg.bayes_factor(a, dict(a, n_data=25))


# ---- 7. error paths ----------------------------------------------------------------------------------------------------------
def test_error_paths(pkg, gpu_engine):
    E = pkg.RsfError
    ok = dict(mean=[1000.0], chol=[[35.0]], lo=[900.0], hi=[1100.0], n2=10)

    def code(fn, *a, **kw):
        with pytest.raises(E) as ei:
            fn(*a, **kw)
        return ei.value.code

    assert gpu_engine.evidence_propose(**ok)[0].shape == (10, 1)
    assert code(gpu_engine.evidence_propose, **dict(ok, n2=0)) == -1
    assert code(gpu_engine.evidence_propose, **dict(ok, mean=[np.nan])) == -1
    assert code(gpu_engine.evidence_propose, **dict(ok, chol=[[0.0]])) == -1
    assert code(gpu_engine.evidence_propose, **dict(ok, chol=[[-1.0]])) == -1
    assert code(gpu_engine.evidence_propose, **dict(ok, lo=[0.0], transform=["log"])) == -1
    assert code(gpu_engine.evidence_propose, **dict(ok, lo=[1200.0])) == -1
    assert code(gpu_engine.evidence_propose, **dict(ok, offset=-1)) == -1
    m3, lo3, hi3 = [1.0, 2.0, 3.0], [0.0, 1.0, 2.0], [2.0, 3.0, 4.0]
    upper = [[1.0, 0.1, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    assert code(gpu_engine.evidence_propose, m3, upper, lo3, hi3, 10) == -1  # not lower triangular
    assert code(gpu_engine.evidence_logg, np.ones((4, 3)), m3, upper) == -1
    lib, dbl, i32 = gpu_engine.lib, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    m4, L4, t4, out = np.zeros(4), np.eye(4), np.zeros(4, dtype=np.int32), np.zeros(40)
    P = lambda x: x.ctypes.data_as(dbl)
    assert lib.rsf_evidence_propose(gpu_engine._ctx, 10, 4, P(m4), P(L4), t4.ctypes.data_as(i32), P(m4), P(m4 + 1), 0, 0, out.ctypes.data,
                                    out.ctypes.data, out.ctypes.data) == -1  # d > 3
    assert lib.rsf_evidence_logg(gpu_engine._ctx, 10, 4, out.ctypes.data, P(m4), P(L4), t4.ctypes.data_as(i32), out.ctypes.data) == -1
    assert lib.rsf_evidence_logg(gpu_engine._ctx, 0, 1, out.ctypes.data, P(m4), P(L4[:1, :1].copy()), t4.ctypes.data_as(i32), out.ctypes.data) == -1
    # the fused kernel needs a model: RSF_ERR_STATE through the C ABI, and from the wrapper
    assert lib.rsf_evidence_logtarget(gpu_engine._ctx, 4, 1, out.ctypes.data, out.ctypes.data, 12.0, P(m4), P(m4 + 1), t4.ctypes.data_as(i32),
                                      out.ctypes.data, out.ctypes.data) == -3
    with pytest.raises(E, match="set_model"):
        gpu_engine.evidence_logtarget(np.full(4, 1000.0), np.zeros(500), 0.0, 1e4, np.zeros(4))
    model = pkg.RateStateModel(number_time_steps=50)
    gpu_engine.set_model(model, 1)
    nout = gpu_engine.nout
    args = (np.full(4, 1000.0), np.zeros(nout), 0.0, 1e4, np.zeros(4))
    assert np.isfinite(gpu_engine.evidence_logtarget(*args)).all()
    assert code(gpu_engine.evidence_logtarget, *args, transform=["log"]) == -1  # lo = 0
    assert code(gpu_engine.evidence_logtarget, *args, shape=0.0) == -1
    assert code(gpu_engine.evidence_logtarget, np.ones((4, 2)), *args[1:]) == -1  # d = 2
    assert lib.rsf_evidence_logtarget(gpu_engine._ctx, 0, 1, out.ctypes.data, out.ctypes.data, 12.0, P(m4), P(m4 + 1), t4.ctypes.data_as(i32),
                                      out.ctypes.data, out.ctypes.data) == -1
    model.integrator = "dop853"
    gpu_engine.set_model(model, 1)
    assert code(gpu_engine.evidence_logtarget, *args) == -5
    # a posterior draw outside the support, a NaN among the proposal draws, a bad r
    assert code(gpu_engine.evidence_partials, [0.0, -np.inf], [0.0], 0.0, 1.0) == -1
    assert code(gpu_engine.evidence_partials, [0.0], [np.nan], 0.0, 1.0) == -1
    assert code(gpu_engine.evidence_partials, [0.0], [0.0], 0.0, 0.0) == -1
    part = gpu_engine.evidence_partials([0.0, 0.1], [0.0, 0.2], 0.0, 1.0)
    assert code(gpu_engine.evidence_finish, part, 1.0, 0.0, ess_factor=0.0) == -1
    assert code(gpu_engine.evidence_finish, part, 1.0, 0.0, ess_factor=1.5) == -1
    assert code(gpu_engine.evidence_finish, part, 1.0, 0.0, shape=12.0, lo=[1.0], hi=[1.0]) == -1
