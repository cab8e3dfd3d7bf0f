"""
Specification of the adaptive proposal of adapt_mode = "am" in NumPy long double (TEST INFRASTRUCTURE ONLY, no GPU), and the one
procedure that holds an engine to it — the CPU checker in tests/test_adapt_reference.py, the GPU in tests/test_gpu_adapt.py.

The proposal.  Iterations count from rsf_mcmc_init, across launches: iteration t = 0, 1, ... leaves the state q_(t+1) (row t of the
trace), q_0 is the start.  The history of a chain is q_1 .. q_n — every iteration's state, also a rejected or out-of-bounds one's;
q_0 is not part of it (the library uses it as the shift of its sums only).  With the interval I, after iteration k - 1 for every
multiple k of I (a "boundary") the chain's covariance becomes
    V_k = (2.38^2 / d) (cov(q_1 .. q_k, ddof 1) + diag(eps)),   eps_p = (1e-6 (hi_p - lo_p))^2,
and iteration t proposes q + L z with L the lower Cholesky factor of the V in force: the one the chain was given (rsf_mcmc_init's, or
rsf_mcmc_set_state's, which does not touch the history) before the first boundary after it, V_k with k = I floor(t / I) from then
on; z = the normals of (seed, chain_offset + chain, t) (variates_reference.draws; smc_reference.normals in float64).

The bound.  The library forms cov from sums shifted about q_0: sum (q - q_0) and sum (q - q_0)(q - q_0)^T.  Shifted sums lose
accuracy with the distance of the mean from the shift (Chan, Golub & LeVeque 1983: the relative error is of order n eps (1 + kappa)),
so with kappa_k = max_p (mean_p - q_0p)^2 / var_p of the history (mean, var of q_1 .. q_k; a parameter whose k samples are all equal
has var_p = 0: kappa_p = 0 if they equal q_0p, where every term of the sums is exactly zero, and (mean_p - q_0p)^2 / eps_p otherwise,
eps_p being all the variance V_pp then has) the library is held to
    |V - V_k|_pr <= 4 k eps (1 + kappa_k) sqrt(V_pp V_rr),   eps = 2^-52,
and the steps it takes, at d = 1, to   |dq - L z| <= (4 k eps (1 + kappa_k) + 1e-12) sqrt(V) |z|   (1e-12 alone before the first boundary),
plus the rounding of the stored q itself (step_ratio).  At d = 3 an error of V reaches the factor amplified by the conditioning of
the factorisation, which the first windows make large — a history of seven iterations holds three or four distinct points, its
covariance is singular but for eps, and the condition number cond_2(R) of the correlation matrix R = D^-1 V D^-1, D = sqrt(diag V),
is 1e9 .. 1e11 there.  With |dV_pr| <= delta sqrt(V_pp V_rr): ||dR||_F <= d delta, ||R||_2 >= 1, and the first-order perturbation bound
of the Cholesky factor (Sun 1991; Higham, Accuracy and Stability of Numerical Algorithms, 10.8) gives for the rows of the factor
    ||dL_p.||_2 <= amp delta sqrt(V_pp),   amp = max(1, d^1.5 / sqrt(2) cond_2(R))   (d = 1: amp = 1),
so the step's tolerance is (amp (delta + (d + 1) eps) + 1e-12) sqrt(V_pp) ||z||_2 with delta = 4 k eps (1 + kappa_k) for a window and 0 for
a given V; (d + 1) eps is the backward error of the float64 factorisation itself (Higham 10.3).
"""
import numpy as np

import variates_reference as vr
from conftest import synthetic_data

LD = np.longdouble
EPS = 2.0 ** -52
BOUND_CONSTANT = 4.0
STEP_SLACK = 1e-12
BOX_LO, BOX_HI = [0.0, 0.005, 0.005], [1.0e4, 0.02, 0.03]  # tests/test_gpu_parity.py's
CHAIN_OFFSET = 100
SEED = 11

# precision, d, chains (None: a workgroup's worth of float32 chains, then its first slot again and 37 of its second), interval,
# launches, and what the engine is made with / the model carries.  In every case a launch starts between two boundaries and a launch
# spans two; in a - e one also ends on a boundary (14, 16, 20 iterations), so that the next starts with the window just stored.
CASES = {
    "a": dict(precision="float64", d=1, chains=130, interval=7, launches=(5, 9, 11)),
    "b": dict(precision="float64", d=3, chains=130, interval=7, launches=(5, 9, 11)),
    "c": dict(precision="float64", d=3, chains=70, interval=4, launches=(3, 3, 10), block_threads=64),
    "d": dict(precision="float32", d=1, chains=None, interval=5, launches=(4, 7, 9)),
    "e": dict(precision="float32", d=3, chains=None, interval=7, launches=(5, 9, 11)),
    "f": dict(precision="float64", d=1, chains=64, interval=5, launches=(3, 8), integrator="dop853"),
}
V3 = np.diag([25.0 ** 2, 1e-4 ** 2, 1e-4 ** 2])  # tests/test_gpu_parity.py: test_edge_cases_and_call_order


def chol_lower(V):
    """V (C, d, d) long double → (L (C, d, d), ok (C,)): the lower Cholesky factor, ok where every pivot is positive"""
    V = np.asarray(V, dtype=LD)
    C, d, _ = V.shape
    L, ok = np.zeros_like(V), np.ones(C, dtype=bool)
    for j in range(d):
        s = V[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
        ok &= s > 0
        L[:, j, j] = np.sqrt(np.where(s > 0, s, 1))
        for i in range(j + 1, d):
            L[:, i, j] = (V[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)) / L[:, j, j]
    return L, ok


def windows(tq, q0, lo, hi, interval):
    """tq (N, C, d): the trace from rsf_mcmc_init on; q0 (C, d) → {k: dict(V, L (C, d, d) long double, kappa (C,), bound (C,) float64)} for
    amp (C,)) for every boundary k = interval, 2 interval, ... <= N"""
    tq, q0 = np.asarray(tq, dtype=LD), np.asarray(q0, dtype=LD)
    N, C, d = tq.shape
    eps = (LD(1e-6) * (np.asarray(hi, dtype=LD) - np.asarray(lo, dtype=LD))[:d]) ** 2
    out = {}
    for k in range(interval, N + 1, interval):
        h = tq[:k]
        mean = h.sum(axis=0) / k
        dev = h - mean
        cov = np.einsum("ncp,ncr->cpr", dev, dev) / (k - 1)
        V = (LD(2.38) ** 2 / d) * (cov + np.eye(d, dtype=LD) * eps)
        L, ok = chol_lower(V)
        assert k >= 2 and ok.all(), "with eps > 0 every history has a factor"
        var, shift2 = np.diagonal(cov, axis1=1, axis2=2), (mean - q0) ** 2
        kappa = np.where(var > 0, shift2 / np.where(var > 0, var, 1), np.where(shift2 > 0, shift2 / eps, 0)).max(axis=1).astype(np.float64)
        out[k] = dict(V=V, L=L, kappa=kappa, bound=BOUND_CONSTANT * k * EPS * (1 + kappa), amp=amplification(V))
    return out


def amplification(V):
    """amp of the module docstring for every V (C, d, d) → (C,)"""
    V = np.asarray(V, dtype=np.float64)
    d = V.shape[1]
    if d == 1:
        return np.ones(V.shape[0])
    sd = np.sqrt(np.diagonal(V, axis1=1, axis2=2))
    return np.maximum(1.0, d ** 1.5 / np.sqrt(2.0) * np.linalg.cond(V / (sd[:, :, None] * sd[:, None, :])))


def v_ratio(V, win):
    """the largest |V - V_k|_pr / (bound sqrt(V_pp V_rr)) of every chain → (C,)"""
    sd = np.sqrt(np.diagonal(win["V"], axis1=1, axis2=2))
    err = np.abs(np.asarray(V, dtype=LD) - win["V"]) / (sd[:, :, None] * sd[:, None, :])
    return (err.max(axis=(1, 2)) / win["bound"]).astype(np.float64)


def normals(gid, t, d):
    """the normals of iteration t and the bound their float64 values are held to (tests/variates_reference.py) → (z, z_bound) (C, d)"""
    w = vr.draws(SEED, gid, t, d)
    return w["z"], vr.z_bound(w["z"], w["r"])


def step_ratio(q_prev, q_new, L, zz, bound):
    """|(q_new - q_prev) - L z|_p over its tolerance, the largest over p → (C,).  The tolerance: (bound + 1e-12) sqrt(V_pp) ||z||_2 with
    bound = amp (delta + (d + 1) eps) of the module docstring, plus
    what storing q_new in float64 costs whatever the factor — component p is q_p plus p + 1 products, each addition rounded once:
    (p + 1) (eps / 2) (|q_prev,p| + sum_r |L_pr z_r|).  (Without that term a step with a small |z| — a step of 0.3 from Dc = 2000 —
    would be held to less than the spacing of the float64 numbers it lands among.)  And what the normals' own rounding allows:
    sum_r |L_pr| eps (4 |z_r| + 2 r_r), z and its bound from normals() — absolute in z, so it too matters for a small |z| only."""
    z, zb = zz
    L, z, q_prev = np.asarray(L, dtype=LD), np.asarray(z, dtype=LD), np.asarray(q_prev, dtype=LD)
    step = np.einsum("cpr,cr->cp", L, z)
    sd = np.sqrt((L ** 2).sum(axis=2))  # sqrt(V_pp)
    tol = (np.asarray(bound, dtype=LD) + STEP_SLACK)[:, None] * sd * np.sqrt((z ** 2).sum(axis=1))[:, None]
    tol = tol + (1 + np.arange(L.shape[1])) * (EPS / 2) * (np.abs(q_prev) + np.einsum("cpr,cr->cp", np.abs(L), np.abs(z)))
    tol = tol + np.einsum("cpr,cr->cp", np.abs(L), np.asarray(zb, dtype=LD))
    return (np.abs(np.asarray(q_new, dtype=LD) - q_prev - step) / tol).max(axis=1).astype(np.float64)


def model_of(oracle_mod, case):
    m = oracle_mod.ModelSpec(100)
    m.precision, m.integrator = case["precision"], case.get("integrator", "rk4")
    return m


def chains_of(engine, case):
    if case["chains"] is not None:
        return case["chains"]
    # float32: chain w 2 B + s B + t is slot s of lane t of workgroup w (B threads): workgroup 0 whole — every lane carries two chains —
    # and workgroup 1 with its first slot full and 37 chains in its second
    return 3 * engine.block_threads + 37


def starts(C, d):
    rng = np.random.default_rng(17)
    return np.column_stack([np.linspace(600.0, 2400.0, C), rng.uniform(0.010, 0.012, C), rng.uniform(0.013, 0.015, C)])[:, :d].copy()


def run_case(engine, oracle_mod, case, set_V3_after=None, label=""):
    """Initialise `engine` for `case`, run its launches and check, after every launch and over the whole trace, assertions 1, 2, 4 and 5
    of the specification above (3 with set_V3_after = the index of the launch after which set_state(V = V3) is called).
    → dict of what was measured."""
    d, interval, launches = case["d"], case["interval"], case["launches"]
    engine.set_model(model_of(oracle_mod, case), 1)
    data = synthetic_data(engine)
    C = chains_of(engine, case)
    q0 = starts(C, d)
    lo, hi = BOX_LO[:d], BOX_HI[:d]
    kw = dict(seed=SEED, chain_offset=CHAIN_OFFSET, prior_len=3 if d == 1 else 0, adapt_interval=interval, fd_rel_step=1e-6 if d == 1 else 1e-4)
    engine.mcmc_init(q0, data, lo, hi, adapt_mode="am", **kw)
    V_init = np.asarray(engine.get_state()[3]).copy()
    assert np.isfinite(V_init).all()
    V_set, set_at = np.tile(V3, (C, 1, 1)), None  # set_state(V = V3) before iteration set_at
    tq, ta, V_after = [], [], []
    for j, n in enumerate(launches):
        q, _, a = engine.mcmc_run(n)
        tq.append(np.asarray(q).copy())
        ta.append(np.asarray(a).copy())
        V_after.append(np.asarray(engine.get_state()[3]).copy())
        if set_V3_after == j:
            set_at = sum(launches[:j + 1])
            assert d == 3 and set_at % interval, "set_state between two boundaries"
            engine.set_state(V=V_set)
            np.testing.assert_array_equal(np.asarray(engine.get_state()[3]), V_set)
    tq, ta = np.concatenate(tq), np.concatenate(ta).astype(bool)
    N = tq.shape[0]
    win = windows(tq, q0, lo, hi, interval)
    res = dict(C=C, N=N, boundaries=sorted(win), kappa_max=max(float(w["kappa"].max()) for w in win.values()))

    def in_force(t):
        """what iteration t proposes with → (k, V or None): the last boundary's window k > 0, or a V the chain was given (k = 0)"""
        k = t // interval * interval
        if set_at is not None and t >= set_at and set_at > k:
            return 0, V_set
        return (k, None) if k else (0, V_init)

    # 1. the covariance after every launch: V_k of the last boundary reached, within the bound; a given V bit for bit until then
    ratios, done, spans = [], 0, False
    for j, n in enumerate(launches):
        spans |= (done + n) // interval - done // interval >= 2
        done += n
        k, V_then = in_force(done) if set_V3_after != j else in_force(done - 1)  # (V_after[j] was read before set_state)
        if k == 0:
            np.testing.assert_array_equal(V_after[j], V_then, err_msg=f"{label}: V changed without a boundary (launch {j})")
        else:
            r = v_ratio(V_after[j], win[k])
            ratios.append(r)
            c = int(np.argmax(r))
            print(f"{label} after launch {j} ({done} iterations, boundary {k}): V / bound max {r.max():.3f} median {np.median(r):.2e} "
                  f"(chain {c}: kappa {win[k]['kappa'][c]:.2e}); kappa max {win[k]['kappa'].max():.2e}")
            assert r.max() <= 1.0, f"{label}: chain {c} holds a V at {r.max():.3f} of its bound after {done} iterations"
    assert spans, "one launch spans two boundaries"
    res["v_ratio"] = float(np.max([r.max() for r in ratios]))
    res["v_ratio_median"] = float(np.median(np.concatenate(ratios)))

    # 2. the proposal in force, from the trace: every accepted step is L z with the factor of the window then in force
    gid = CHAIN_OFFSET + np.arange(C, dtype=np.uint64)
    L_of, bound_of = {}, {}
    for name, V in (("init", V_init), ("set", V_set)):
        L_of[name], ok = chol_lower(V.astype(LD))
        bound_of[name] = amplification(V) * (V.shape[1] + 1) * EPS
        assert ok.all()
    worst, compared, first_of_launch, given_steps = 0.0, 0, 0.0, 0
    launch_starts = set(np.cumsum(launches)[:-1].tolist())
    for t in range(N):
        k, V_then = in_force(t)
        given = "set" if V_then is V_set else "init"
        L, bound = (win[k]["L"], win[k]["amp"] * (win[k]["bound"] + (d + 1) * EPS)) if k else (L_of[given], bound_of[given])
        acc = ta[t]
        if not acc.any():
            continue
        z, zb = normals(gid, t, d)
        r = step_ratio((tq[t - 1] if t else q0)[acc], tq[t][acc], L[acc], (z[acc], zb[acc]), np.asarray(bound)[acc])
        worst = max(worst, float(r.max()))
        if t in launch_starts:
            first_of_launch = max(first_of_launch, float(r.max()))
        compared += int(acc.sum())
        given_steps += int(acc.sum()) if V_then is V_set else 0
        assert r.max() <= 1.0, f"{label}: iteration {t} (window {k}), chain {int(np.flatnonzero(acc)[np.argmax(r)])}: step off by {r.max():.3e} of its tolerance"
    print(f"{label}: {compared} accepted steps of {N * C} iterations compared with L z, largest ratio to the tolerance {worst:.3e} "
          f"(first iteration of a launch: {first_of_launch:.3e})")
    assert compared >= N * C / 4, f"{label}: only {compared} of {N * C} iterations accepted"
    res.update(step_ratio=worst, step_ratio_launch_start=first_of_launch, compared=compared)
    if set_at is not None:  # 3. the steps up to the next boundary are chol(V3) z
        print(f"{label}: {given_steps} accepted steps under set_state(V = V3), iterations {set_at} .. {(set_at // interval + 1) * interval - 1}")
        assert given_steps >= C // 4
        res["v3_steps"] = given_steps

    # 4. the float32 sampler's two chains of a lane hold their own windows: wherever the histories of a pair differ, so do their V
    if case["precision"] == "float32":
        B = engine.block_threads
        pairs = [(t, B + t) for t in range(B)] + [(2 * B + t, 3 * B + t) for t in range(37)] + [(2 * i, 2 * i + 1) for i in range(C // 2)]
        res["pairs"], done = 0, 0
        for j, n in enumerate(launches):
            done += n
            k = done // interval * interval
            if k == 0:
                continue
            Vk = np.asarray(win[k]["V"], dtype=np.float64)
            differ = [(a, b) for a, b in pairs if not np.array_equal(Vk[a], Vk[b])]
            same = [(a, b) for a, b in differ if np.array_equal(V_after[j][a], V_after[j][b])]
            print(f"{label} after launch {j}: {len(differ)} of {len(pairs)} chain pairs (the two slots of a lane, and neighbours) have different "
                  f"histories; {len(same)} of them hold equal V")
            assert len(differ) >= len(pairs) // 2 and not same
            res["pairs"] += len(differ)
        assert res["pairs"] > 0

    # 5. frozen: re-initialised with adapt_mode none from the adapted state, V stays bit for bit and the steps are its factor's
    state = [np.asarray(x).copy() for x in engine.get_state()]
    engine.mcmc_init(state[0], data, lo, hi, adapt_mode="none", **kw)
    engine.set_state(*state)
    np.testing.assert_array_equal(np.asarray(engine.get_state()[3]), state[3])
    fq, _, fa = engine.mcmc_run(2 * interval)
    fq, fa = np.asarray(fq), np.asarray(fa).astype(bool)
    np.testing.assert_array_equal(np.asarray(engine.get_state()[3]), state[3], err_msg=f"{label}: V moved under adapt_mode none")
    Lf, ok = chol_lower(state[3].astype(LD))
    assert ok.all()
    frozen = 0.0
    for t in range(2 * interval):
        acc = fa[t]
        if acc.any():
            frozen = max(frozen, float(step_ratio((fq[t - 1] if t else state[0])[acc], fq[t][acc], Lf[acc], tuple(x[acc] for x in normals(gid, t, d)),
                                                  (amplification(state[3]) * (d + 1) * EPS)[acc]).max()))
    print(f"{label}: frozen proposal over {2 * interval} iterations: V unchanged bit for bit, steps within {frozen:.3e} of their tolerance")
    assert frozen <= 1.0 and fa.sum() > 0
    res["frozen_step_ratio"] = frozen
    return res
