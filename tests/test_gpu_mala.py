"""
GPU tests of the Gauss-Newton manifold MALA sampler (include/rsf_mala.h: rsf_mala_run / _propose / _accept; Engine.mala,
Engine.mala_from_residuals, MCMC.sample_mala, RSF.inference_mala) against the specification tests/mala_reference.py and the exact
target tests/posterior_reference.py.

1. the split path against the specification, one iteration at a time from the specification's state: closed forms at d = 1, 2, 3
   and rows constructed for every way an iteration can end.
2. the fused kernel against the split path on the real model, bit for bit.
3. the sampler keeps its target: closed forms and the real model at d = 1 and d = 3, held to the quadrature by check().
4. counters and trace.  5. chain identity.  6. the front ends.  7. error codes.
Every test prints what it measured before it asserts.
"""
import numpy as np
import pytest

import mala_reference as M
import posterior_reference as R
import smc_reference as S
from test_fit_reference import checker_problem
from test_gpu_posterior import BOX1, HI3, LO3, _reference

pytestmark = pytest.mark.gpu

_CACHE = {}
NAMES = ("q", "ssq", "g", "H", "accepted", "outbox", "stuck")


def _model(pkg, nsteps=500, substeps=1, damping=True):
    m = pkg.RateStateModel(number_time_steps=nsteps)
    m.RadiationDamping = damping
    m.substeps = substeps
    return m


def _draws(seed, offset, n, it, d):
    """the NumPy restatement of rsf_mcmc_draws (tests/smc_reference.py): u is exact, z differs from the device's in its last bits"""
    ids = offset + np.arange(n, dtype=np.uint64)
    return S.normals(seed, ids, it, d), S.accept_uniforms(seed, ids, it)


def _bits(arrays):
    return [np.ascontiguousarray(x).view(np.int32 if x.dtype.itemsize == 4 else np.int64) for x in arrays]


# ---- 1. the split path against the specification ---------------------------------------------------------------------------------------
def _split_against_specification(eng, tag, st, new_fn, lo, hi, eps, lam, shape, n_iter, seed=11, offset=5):
    """n_iter iterations of the specification; at each, rsf_mala_propose and rsf_mala_accept start from a copy of the
    specification's state and are fed new_fn at the SPECIFICATION's proposal (the GPU's lies within 1e-13 of the box width of it,
    asserted).  -> (chain-iterations excluded as ties, decisions compared, accepted)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    n, d = st["q"].shape
    excluded = compared = accepted = 0
    for it in range(1, n_iter + 1):
        gs, before = ({k: v.copy() for k, v in st.items()} for _ in range(2))
        z, u = _draws(seed, offset, n, it, d)
        out = M.iterate(new_fn, st, z, u, lo, hi, eps, lam, shape)  # st moves on; gs is the state before
        kw = dict(shape=shape, eps=eps, lam=lam, seed=seed, offset=offset, iteration=it)
        qn, inb, stk = eng.mala_propose(gs["q"], gs["ssq"], gs["g"], gs["H"], lo, hi, **kw)
        np.testing.assert_array_equal(inb.astype(bool), out["inbox"], err_msg=f"{tag} iteration {it}: inbox")
        np.testing.assert_array_equal(stk.astype(bool), out["stuck"], err_msg=f"{tag} iteration {it}: stuck")
        e = float((np.abs(qn - out["qn"]) / (hi - lo)).max())
        np.testing.assert_array_equal(qn[~out["inbox"]], gs["q"][~out["inbox"]])  # no proposal inside the box: the chain's own point
        eng.mala_accept(gs["q"], gs["ssq"], gs["g"], gs["H"], lo, hi, qn, inb, out["ssq_n"], out["g_n"], out["H_n"], gs["accepted"], gs["outbox"],
                        gs["stuck"], **kw)
        got = gs["accepted"] > st["accepted"] - out["accepted"]
        with np.errstate(invalid="ignore"):
            tie = out["inbox"] & np.isfinite(out["margin"]) & (np.abs(out["margin"]) <= 1e-9 * (1 + np.abs(out["log_alpha"])))
        excluded += int(tie.sum())
        compared += int((out["inbox"] & ~tie).sum())
        accepted += int(out["accepted"].sum())
        print(f"{tag} iteration {it}: q_new error / box width {e:.2e}, inside {int(out['inbox'].sum())}, stuck {int(out['stuck'].sum())}, accepted "
              f"{int(out['accepted'].sum())}, ties {int(tie.sum())}, smallest |margin| {np.nanmin(np.abs(out['margin'])) if out['inbox'].any() else np.nan:.2e}")
        assert e <= 1e-13, (tag, it, e)
        np.testing.assert_array_equal(got[~tie], out["accepted"][~tie], err_msg=f"{tag} iteration {it}: decisions")
        # an accepted state is the supplied sums' bits and the GPU's own proposal; a chain that did not move keeps its bits
        for k, new in (("ssq", out["ssq_n"]), ("g", out["g_n"]), ("H", out["H_n"]), ("q", qn)):
            assert gs[k][got].tobytes() == np.ascontiguousarray(new[got]).tobytes(), (tag, it, k)
        same = ~got & ~out["accepted"]
        for k in ("q", "ssq", "g", "H"):
            assert gs[k][same].tobytes() == before[k][same].tobytes(), (tag, it, k)
        keep = ~tie
        np.testing.assert_array_equal(gs["outbox"][keep], st["outbox"][keep], err_msg=f"{tag} iteration {it}: outbox")
        np.testing.assert_array_equal(gs["stuck"][keep], st["stuck"][keep], err_msg=f"{tag} iteration {it}: stuck count")
    return excluded, compared, accepted


CLOSED2 = dict(S0=1.0, q0=[1.0, 2.0], K=[[4.0, 1.0], [1.0, 3.0]], lo=[0.0, 1.4], hi=[10.0, 2.6], shape=12.0)


def _closed(d):
    c = CLOSED2 if d == 2 else R.CLOSED[d]
    K, q0 = np.asarray(c["K"], dtype=np.float64), np.asarray(c["q0"], dtype=np.float64)
    fn = R.quadratic_ssq(c["S0"], c["q0"], c["K"])

    def normal(q):  # a metric that depends on the position (tests/test_mala_reference.py)
        f = (1.0 + 0.5 * np.sin(3.0 * q[:, 0])) ** 2
        return fn(*q.T), (q - q0) @ K.T, K[None] * f[:, None, None]

    return c, normal


@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_split_path_against_the_specification_on_closed_forms(gpu_engine, d, lam):
    c, normal = _closed(d)
    rng = np.random.default_rng([21, d])
    n = 257  # a second, partial workgroup of the split kernels
    sd = np.sqrt(np.diag(np.linalg.inv(np.asarray(c["K"]))) * c["S0"] / (2 * c["shape"] - d))
    q0 = np.clip(np.asarray(c["q0"]) + 1.5 * sd * rng.standard_normal((n, d)), np.asarray(c["lo"]) + 1e-3, np.asarray(c["hi"]) - 1e-3)
    st = M.new_state(q0, *normal(q0))
    excluded, compared, accepted = _split_against_specification(gpu_engine, f"closed d {d} lam {lam}", st, normal, c["lo"], c["hi"], 1.0, lam, c["shape"], 4)
    print(f"closed d {d} lam {lam}: {compared} decisions compared, {accepted} accepted, {excluded} excluded as ties; counters {st['accepted'].sum()} "
          f"{st['outbox'].sum()} {st['stuck'].sum()}")
    assert excluded <= 1 and compared > 0.5 * 4 * n and 0.3 * compared < accepted < compared and st["outbox"].sum() > 0 and st["stuck"].sum() == 0


def test_split_path_on_constructed_rows(gpu_engine):
    c = R.CLOSED[3]
    K, q0, lo, hi = np.asarray(c["K"]), np.asarray(c["q0"]), np.asarray(c["lo"]), np.asarray(c["hi"])
    fn = R.quadratic_ssq(c["S0"], c["q0"], c["K"])
    mid, eps = np.array([1.0, 2.0, 2.8]), 0.3
    rows = []  # (q, g, H, what the solve at the proposal returns)
    for p in range(3):  # a proposal outside each face: the drift -(eps^2 / 2) A^-1 g is 4.5 along the axis, the noise about 0.03
        for sign in (+1.0, -1.0):
            q = mid.copy()
            if p == 0 and sign < 0:
                q[0] = 9.0  # the upper face of the first coordinate lies at 10
            rows.append((q, K @ (100.0 * sign * np.eye(3)[p]), K, "ordinary"))
    rows.append((mid, K @ (mid - q0), -K, "ordinary"))            # the factor at the current point fails: stuck
    rows.append((mid, K @ (mid - q0), K * np.nan, "ordinary"))    # ... on a NaN
    for what in ("factor", "inf", "nan", "zero", "negative", "ordinary"):  # a proposal inside (nine noise SD from the nearest face)
        rows.append((mid, K @ (mid - q0), K, what))
    n = len(rows)
    what = np.array([r[3] for r in rows])

    def new_fn(qn):
        ssq = fn(*qn.T)
        ssq[what == "inf"], ssq[what == "nan"], ssq[what == "zero"], ssq[what == "negative"] = np.inf, np.nan, 0.0, -1.0
        H = np.tile(K, (n, 1, 1))
        H[what == "factor"] = -K
        return ssq, (qn - q0) @ K.T, H

    for lam in (0.0, 1e-3):
        q = np.array([r[0] for r in rows])
        st = M.new_state(q, fn(*q.T), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]))
        excluded, compared, accepted = _split_against_specification(gpu_engine, f"constructed lam {lam}", st, new_fn, lo, hi, eps, lam, c["shape"], 1)
        print(f"constructed lam {lam}: accepted {st['accepted'].tolist()} outbox {st['outbox'].tolist()} stuck {st['stuck'].tolist()}")
        assert excluded == 0 and compared == 6
        assert st["outbox"].tolist() == [1] * 6 + [0] * 8 and st["stuck"].tolist() == [0] * 6 + [1, 1] + [0] * 6
        assert st["accepted"].tolist() == [0] * 13 + [1]  # only the ordinary row moves


# ---- 2. fused against split on the real model ---------------------------------------------------------------------------------------
def _observation(pkg, cpu_engine, nsteps, substeps, damping, truths):
    key = (nsteps, substeps, damping, truths)
    if key not in _CACHE:
        cpu_engine.set_model(_model(pkg, nsteps, substeps, damping), substeps)
        acc = np.asarray(cpu_engine.forward(list(truths))[1]).T
        _CACHE[key] = acc + 0.01 * np.abs(acc).max() * np.random.default_rng(3).standard_normal(acc.shape)
    return _CACHE[key]


def _starts(d, n, seed=7):
    rng = np.random.default_rng(seed)
    q = np.linspace(900.0, 1100.0, n)[:, None]
    if d == 3:
        q = np.concatenate([q, 0.011 + 0.002 * rng.random((n, 1)), 0.014 + 0.002 * rng.random((n, 1))], axis=1)
    return q


def _gpu_state(eng, q0, data, fd):
    ssq, g, H = eng.fit_normal(q0, data, fd)
    n = q0.shape[0]
    return {"q": q0.copy(), "ssq": ssq, "g": g, "H": H, **{k: np.zeros(n, dtype=np.int32) for k in ("accepted", "outbox", "stuck")}}


#          name: (nsteps, substeps, d, n, observation rows, workgroup threads, damping)
FUSED_CASES = {
    "d1_n133_partial_workgroup": (500, 1, 1, 133, 1, 0, True),   # 128 pairs fill a workgroup of 256; the pairs of a wave end at a wave edge
    "d3_n17": (500, 1, 3, 17, 1, 0, True),                       # 16 quads fill a wave
    "d1_two_rows": (500, 1, 1, 128, 2, 64, True),                # two observation series of 64 chains, workgroups of 64 threads
    "d3_two_rows": (500, 1, 3, 128, 2, 64, True),
    "d1_two_chunks": (800, 4, 1, 5, 1, 0, True),                 # kc < nout - 1: the table is staged in two chunks
    "d1_no_damping": (500, 1, 1, 5, 1, 0, False),
}


@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_fused_against_split_on_the_real_model(pkg, cpu_engine, name):
    nsteps, sub, d, n, G, block, damping = FUSED_CASES[name]
    data = _observation(pkg, cpu_engine, nsteps, sub, damping, (1000.0, 960.0)[:G])
    data = data if G > 1 else data[0]
    lo, hi, fd = (BOX1[0], BOX1[1], 1e-6) if d == 1 else (LO3, HI3, 1e-4)
    q0 = _starts(d, n)
    kw = dict(eps=1.0, lam=1e-3, seed=9, offset=100)
    with pkg.Engine(mem="host", block_threads=block) as eng:
        eng.set_model(_model(pkg, nsteps, sub, damping), sub)
        fused = _gpu_state(eng, q0, data, fd)
        split = {k: v.copy() for k, v in fused.items()}
        once = {k: v.copy() for k, v in fused.items()}
        rows = []
        for it in range(1, 5):
            tq, ts = eng.mala_run(*(fused[k] for k in ("q", "ssq", "g", "H")), data, lo, hi, 1, *(fused[k] for k in NAMES[4:]), iter0=it, fd_rel_step=fd,
                                  trace=True, **kw)
            rows.append((tq[0], ts[0]))
            qn, inb, stk = eng.mala_propose(split["q"], split["ssq"], split["g"], split["H"], lo, hi, 0.5 * eng.nout, iteration=it, **kw)
            s_n, g_n, h_n = eng.fit_normal(qn, data, fd)
            eng.mala_accept(split["q"], split["ssq"], split["g"], split["H"], lo, hi, qn, inb, s_n, g_n, h_n, *(split[k] for k in NAMES[4:]), 0.5 * eng.nout,
                            iteration=it, **kw)
            same = [np.array_equal(a, b) for a, b in zip(_bits(fused[k] for k in NAMES), _bits(split[k] for k in NAMES))]
            print(f"{name} iteration {it}: inside {int(inb.sum())} stuck {int(stk.sum())} accepted so far {int(fused['accepted'].sum())} of {it * n}, "
                  f"bit-identical {dict(zip(NAMES, same))}")
            assert all(same), (name, it, dict(zip(NAMES, same)))
            # the trace row is the state after the iteration
            assert tq[0].tobytes() == fused["q"].tobytes() and ts[0].tobytes() == fused["ssq"].tobytes()
        assert (fused["accepted"] + fused["outbox"] + fused["stuck"] <= 4).all() and fused["accepted"].sum() > 0
        # four iterations inside one launch: the bits of four launches of one, the trace rows too
        tq, ts = eng.mala_run(*(once[k] for k in ("q", "ssq", "g", "H")), data, lo, hi, 4, *(once[k] for k in NAMES[4:]), iter0=1, fd_rel_step=fd, trace=True,
                              **kw)
        for a, b in zip(_bits(once[k] for k in NAMES), _bits(fused[k] for k in NAMES)):
            np.testing.assert_array_equal(a, b)
        for k in range(4):
            assert tq[k].tobytes() == rows[k][0].tobytes() and ts[k].tobytes() == rows[k][1].tobytes(), k
    # device memory: the same bits
    with pkg.Engine(mem="device", block_threads=block) as dev:
        dev.set_model(_model(pkg, nsteps, sub, damping), sub)
        q = dev._in(q0)
        ssq, g, H = dev.fit_normal(q, data, fd)
        cnt = [dev._ints(np.zeros(n)) for _ in range(3)]
        tq, ts = dev.mala_run(q, ssq, g, H, data, lo, hi, 4, *cnt, iter0=1, fd_rel_step=fd, trace=True, **kw)
        got = [np.asarray(x.cpu()) for x in (q, ssq, g, H, *cnt)]
        for k, a, b in zip(NAMES, _bits(got), _bits(fused[k] for k in NAMES)):
            np.testing.assert_array_equal(a, b, err_msg=f"device memory: {k}")
        assert np.asarray(tq.cpu())[3].tobytes() == fused["q"].tobytes()


# ---- 3. the sampler keeps its target ---------------------------------------------------------------------------------------------------
def _check_kept(tag, ref, res, eng, fails):
    """check() at every kept iteration, sigma^2 from MalaResult.std2 (rsf_smc_std2 of the kept states)"""
    std2 = res.std2(engine=eng, kept=True)
    for r, it in enumerate(res.iterations):
        R.check(f"{tag} it {it}", ref, res.samples[r], std2[r], fails)
    n = res.accepted.shape[0] * res.n_iter
    print(f"{tag}: accepted {res.accepted.sum() / n:.3f}, outside the box {res.outbox.sum() / n:.4f}, stuck {int(res.stuck.sum())}")


@pytest.mark.parametrize("metric", ["residuals", "position_dependent"])
@pytest.mark.parametrize("d", [1, 3])
def test_closed_form_targets_through_the_split_path(gpu_engine, d, metric):
    if ("closed", d) not in _CACHE:
        _CACHE["closed", d] = R.closed_reference(d)
    ref, fn, c = _CACHE["closed", d]
    C, shape = 262144, c["shape"]
    rng = np.random.default_rng([31, d])
    q0 = ref.draw(rng, C)
    Cf = np.linalg.cholesky(np.asarray(c["K"], dtype=np.float64)).T  # K = Cf^T Cf: the residuals (sqrt(S0), Cf (q - q0))
    res_fn = lambda p: np.concatenate([np.full((p.shape[0], 1), np.sqrt(c["S0"])), (p - np.asarray(c["q0"])) @ Cf.T], axis=1)
    kw = dict(res_fn=res_fn, lam=0.0) if metric == "residuals" else dict(res_fn=None, normal_fn=_closed(d)[1], lam=1e-3)
    res = gpu_engine.mala_from_residuals(q0=q0, lo=c["lo"], hi=c["hi"], n_iter=8, shape=shape, seed=17, keep=5, thin=4, **kw)
    assert res.iterations.tolist() == [4, 8]
    fails = []
    _check_kept(f"closed d {d} {metric}", ref, res, gpu_engine, fails)
    np.testing.assert_allclose(res.ssq, fn(*res.q.T), rtol=1e-12)
    assert res.stuck.sum() == 0
    assert not fails, fails


@pytest.mark.parametrize("damping", [True, False])
def test_real_model_target_one_parameter(pkg, cpu_engine, damping):
    ref, data = _reference(pkg, cpu_engine, 1, *BOX1, **({} if damping else {"damping": False}))  # with damping: test_gpu_posterior's own entry
    C = 65536
    q0 = ref.draw(np.random.default_rng(51), C)
    fails = []
    with pkg.Engine(mem="device") as eng:
        eng.set_model(_model(pkg, damping=damping), 1)
        res = eng.mala(q0, data, *BOX1, 20, seed=23, keep=11, thin=10, iters_per_launch=10)
        assert res.iterations.tolist() == [10, 20]
        _check_kept(f"real d 1 damping {damping}", ref, res, eng, fails)
    assert res.stuck.sum() == 0
    assert not fails, fails


# At the default step the proposal is as long as the ridge Dc a = const the Gauss-Newton metric sees, far longer than the box: 99.8 %
# of the proposals leave it and the chains hardly move (measured), so that leg alone would hold a pool that stands still
# to its own start.  eps = 0.01 is the step at which a third of the proposals are accepted and b moves by a posterior SD in twenty
# iterations: the leg in which the Metropolis-Hastings correction at d = 3 is what keeps the target.
@pytest.mark.parametrize("eps", [1.0, 0.01])
def test_real_model_target_three_parameters(pkg, cpu_engine, eps):
    ref, data = _reference(pkg, cpu_engine, 3, LO3, HI3)
    C = 65536
    q0 = ref.draw(np.random.default_rng(52), C)
    fails = []
    with pkg.Engine(mem="device") as eng:
        eng.set_model(_model(pkg), 1)
        res = eng.mala(q0, data, LO3, HI3, 20, eps=eps, seed=24, keep=11, thin=10, iters_per_launch=10)
        assert res.iterations.tolist() == [10, 20]
        _check_kept(f"real d 3 eps {eps}", ref, res, eng, fails)
    moved = np.abs(res.q - q0).mean(axis=0) / np.array([ref.marg[k].sd for k in ("Dc", "a", "b")])
    print(f"real d 3 eps {eps}: mean |q - q0| in posterior SD {moved.tolist()}")
    assert res.stuck.sum() == 0
    assert not fails, fails


# ---- 4. counters and trace ---------------------------------------------------------------------------------------------------------------
def test_counters_and_trace(pkg, gpu_engine, cpu_engine):
    data = checker_problem(pkg, cpu_engine, 1000.0)[0]
    eng = gpu_engine
    eng.set_model(_model(pkg), 1)
    q0 = _starts(1, 40)
    full = eng.mala(q0, data, *BOX1, 12, seed=3, iters_per_launch=5, keep=12)
    assert full.iterations.tolist() == list(range(1, 13)) and full.samples.shape == (12, 40, 1)
    assert (full.accepted + full.outbox + full.stuck <= 12).all() and (full.accepted >= 0).all()
    np.testing.assert_array_equal(full.samples[-1], full.q)
    np.testing.assert_array_equal(full.ssq_trace[-1], full.ssq)
    # a row differs from the one before exactly where the chain accepted: a chain's moves are its accepted count
    rows = np.concatenate([q0[None], full.samples])
    moved = (rows[1:] != rows[:-1]).any(axis=2)
    print(f"counters: accepted {full.accepted.tolist()}, outbox {int(full.outbox.sum())}, stuck {int(full.stuck.sum())}")
    np.testing.assert_array_equal(moved.sum(axis=0), full.accepted)
    s0 = np.asarray(eng.fit_normal(q0, data)[0])
    srows = np.concatenate([s0[None], full.ssq_trace])
    assert ((srows[1:] != srows[:-1]) == moved).all()
    # keep and thin select the stated rows of the same run
    part = eng.mala(q0, data, *BOX1, 12, seed=3, iters_per_launch=5, keep=7, thin=3)
    assert part.iterations.tolist() == [6, 9, 12]
    np.testing.assert_array_equal(part.samples, full.samples[[5, 8, 11]])
    np.testing.assert_array_equal(part.q, full.q)
    # and the launch length does not matter
    other = eng.mala(q0, data, *BOX1, 12, seed=3, iters_per_launch=12, keep=12)
    np.testing.assert_array_equal(other.samples, full.samples)
    np.testing.assert_array_equal(other.accepted, full.accepted)


# ---- 5. chain identity ---------------------------------------------------------------------------------------------------------------------
def test_chain_identity(pkg, gpu_engine, cpu_engine):
    truths = (100.0, 5000.0)
    data = _observation(pkg, cpu_engine, 500, 1, True, truths)
    eng = gpu_engine
    eng.set_model(_model(pkg), 1)
    for d, lo, hi in ((1, *BOX1), (3, LO3, HI3)):
        q0 = _starts(d, 64)
        whole = eng.mala(q0, data[1], lo, hi, 6, seed=4, offset=1000, keep=6)
        for h in (0, 1):
            half = eng.mala(q0[32 * h:32 * h + 32], data[1], lo, hi, 6, seed=4, offset=1000 + 32 * h, keep=6)
            for k in ("q", "ssq", "grad", "jtj", "accepted", "outbox", "stuck"):
                np.testing.assert_array_equal(getattr(half, k), getattr(whole, k)[32 * h:32 * h + 32], err_msg=f"d {d} half {h}: {k}")
            np.testing.assert_array_equal(half.samples, whole.samples[:, 32 * h:32 * h + 32])
    # RSF.inference_mala: its groups are the same groups run one by one (256 chains fill a workgroup: group g's streams start at 256 g)
    problem = pkg.RSF(number_slip_values=2, lowest_slip_value=100.0, largest_slip_value=5000.0, qstart=1000.0, plotfigs=False)
    problem.model = _model(pkg)
    problem.data = data.reshape(-1)
    out = problem.inference_mala(n_chains=256, n_iter=6, start="qstart", seed=8)
    assert sorted(out) == list(truths)
    with pkg.Engine(mem="device") as dev:
        dev.set_model(_model(pkg), 1)
        for g, dc in enumerate(truths):
            one = dev.mala(np.full((256, 1), 1000.0), data[g], *BOX1, 6, seed=8, offset=256 * g, keep=3)
            pool = out[dc]
            print(f"inference_mala Dc_true {dc}: accept rate {pool.accept_rate:.3f}, Dc mean {pool.samples.mean():.2f}")
            np.testing.assert_array_equal(pool.samples, one.samples)
            assert pool.samples.shape == (3, 256, 1) and pool.std2.shape == (3, 256) and pool.accept_rate == one.accept_rate


# ---- 6. the front ends -----------------------------------------------------------------------------------------------------------------------
def test_sample_mala_returns_a_posterior_pool(pkg, cpu_engine):
    ref, data = _reference(pkg, cpu_engine, 1, *BOX1)
    mc = pkg.MCMC(_model(pkg), data, 1000.0, ["Uniform", BOX1[0], BOX1[1]], 1000.0)
    pool = mc.sample_mala(256, 40, start="fit", seed=6)
    assert isinstance(pool, pkg.PosteriorPool) and pool.samples.shape == (20, 256, 1) and pool.std2.shape == (20, 256) and pool.nburn == 20
    diag, rank = pool.diagnostics()[0], pool.rank_diagnostics()[0]
    mg = ref.marg["Dc"]
    z = (pool.samples.mean() - mg.mean) / (mg.sd / np.sqrt(diag["ess"]))
    print(f"sample_mala: accept rate {pool.accept_rate:.3f}, stats { {k: v for k, v in pool.stats.items() if k not in ('ssq', 'fit')} }, Dc mean "
          f"{pool.samples.mean():.2f} against {mg.mean:.2f} (sd {mg.sd:.2f}), ESS {diag['ess']:.0f} (bulk {rank['ess_bulk']:.0f}) of {20 * 256}, "
          f"split R-hat {diag['split_rhat']:.4f}, z {z:+.2f}")
    assert abs(z) < R.Z_MAX
    assert np.isfinite(pool.std2).all() and (pool.std2 > 0).all() and pool.stats["stuck"] == 0 and 0 < pool.accept_rate <= 1
    pool = mc.sample_mala(64, 6, start="qstart", nburn=2, thin=2)
    assert pool.samples.shape == (2, 64, 1) and "fit" not in pool.stats


# ---- 7. contracts -----------------------------------------------------------------------------------------------------------------------------
def test_error_codes(pkg, gpu_engine):
    eng = gpu_engine
    n = 4
    q, data = np.linspace(900.0, 1100.0, n)[:, None], np.zeros(500)
    st = {"q": q.copy(), "ssq": np.ones(n), "g": np.ones((n, 1)), "H": np.ones((n, 1, 1)), **{k: np.zeros(n, dtype=np.int32) for k in NAMES[4:]}}

    def run(**kw):
        a = dict(data=data, lo=BOX1[0], hi=BOX1[1], n_iter=1, eps=1.0, lam=1e-3, shape=250.0, seed=0, offset=0, iter0=1, fd_rel_step=1e-6)
        a.update(kw)
        return eng.mala_run(*(st[k] for k in ("q", "ssq", "g", "H")), a.pop("data"), a.pop("lo"), a.pop("hi"), a.pop("n_iter"), *(st[k] for k in NAMES[4:]), **a)

    def code(call):
        with pytest.raises(pkg.RsfError) as ei:
            call()
        return ei.value.code

    assert code(run) == -3  # no model
    eng.set_model(_model(pkg), 1)
    run()
    for kw in (dict(n_iter=0), dict(n_iter=65), dict(iter0=0), dict(iter0=2 ** 32), dict(offset=-1), dict(eps=0.0), dict(eps=np.inf), dict(lam=-1.0),
               dict(lam=np.nan), dict(shape=0.0), dict(shape=np.nan), dict(fd_rel_step=0.0), dict(fd_rel_step=np.inf), dict(lo=5.0, hi=5.0), dict(hi=np.inf),
               dict(data=np.zeros((3, 500)))):  # 4 chains over 3 series
        assert code(lambda: run(**kw)) == -1, kw
    assert code(lambda: run(data=np.zeros((2, 500)))) == -1  # 2 chains per series: not whole workgroups
    lib, ctx = eng.lib, eng._ctx
    P = lambda a: a.ctypes.data
    dp = lambda v: np.array([v]).ctypes.data_as(pkg._abi._DP)
    ok = [ctx, n, 1, P(st["q"]), P(st["ssq"]), P(st["g"]), P(st["H"]), P(data), 1, dp(0.0), dp(1e4), 1e-6, 1.0, 1e-3, 250.0, 0, 0, 1, 1, P(st["accepted"]),
          P(st["outbox"]), P(st["stuck"]), None, None]
    assert lib.rsf_mala_run(*ok) == 0
    for i, v in ((1, 0), (2, 2), (2, 4), (3, None), (7, None), (9, None), (19, None), (21, None), (22, P(st["q"]))):  # n, d, NULLs, one trace alone
        bad = list(ok)
        bad[i] = v
        assert lib.rsf_mala_run(*bad) == -1, i
    assert lib.rsf_mala_run(None, *ok[1:]) == -1
    # the split calls: d = 1..3, no model needed
    with pkg.Engine(mem="host") as bare:
        qn, inb, stk = bare.mala_propose(st["q"], st["ssq"], st["g"], st["H"], *BOX1, 250.0)
        assert inb.shape == (n,) and stk.shape == (n,)
        z4 = np.ones((n, 4))
        assert code(lambda: bare.mala_propose(z4, st["ssq"], z4, np.ones((n, 4, 4)), [0.0] * 4, [1.0] * 4, 250.0)) == -1
        for kw in (dict(eps=0.0), dict(lam=-1.0), dict(shape=0.0), dict(offset=-1), dict(iteration=0), dict(iteration=2 ** 32)):
            a = dict(shape=250.0)
            a.update(kw)
            assert code(lambda: bare.mala_propose(st["q"], st["ssq"], st["g"], st["H"], *BOX1, **a)) == -1, kw
            assert code(lambda: bare.mala_accept(st["q"], st["ssq"], st["g"], st["H"], *BOX1, qn, inb, st["ssq"], st["g"], st["H"], *(st[k] for k in NAMES[4:]),
                                                 **a)) == -1, kw
        assert code(lambda: bare.mala_propose(st["q"], st["ssq"], st["g"], st["H"], 1.0, 1.0, 250.0)) == -1
        assert bare.lib.rsf_mala_propose(bare._ctx, n, 1, None, None, None, None, dp(0.0), dp(1.0), 1.0, 0.0, 1.0, 0, 0, 1, None, None, None) == -1
        assert b"NULL" in bare.lib.rsf_last_error()
    # the reference's integrator has no MALA; a float32 model gets the float64 solve
    m = _model(pkg)
    m.integrator = "dop853"
    eng.set_model(m, 1)
    assert code(run) == -5
    m = _model(pkg)
    m.precision = "float32"
    eng.set_model(m, 1)
    want = {k: v.copy() for k, v in st.items()}
    run()
    eng.set_model(_model(pkg), 1)
    st, got = want, st
    run()
    for k in NAMES:
        np.testing.assert_array_equal(got[k], st[k], err_msg=k)
