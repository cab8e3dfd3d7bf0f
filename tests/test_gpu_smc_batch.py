"""
GPU tests of the batched SMC populations (include/rsf_smc_batch.h: rsf_smc_batch_init / _logtarget / _weight_sums / _resample /
_move / _std2; Engine.smc_batch).  The specification is the single-population path of include/rsf_smc.h, itself pinned to
tests/smc_reference.py by tests/test_gpu_smc.py: every population of a batched call must equal, BIT FOR BIT, the single call with
that population's seed, offset, data row and parameters.  No tolerance anywhere: every comparison is assert_array_equal.

Shapes: nsteps 500, n = 1000 particles (a tail in the last wave, and in the last 2048-weight tile of the scan, of which n = 2500
has two), P = 3 populations.
"""
import ctypes

import numpy as np
import pytest

import smc_cases as cases

pytestmark = pytest.mark.gpu

N, P = 1000, 3
SEEDS, OFFSETS = [5, 6, 2 ** 40 + 1], [0, cases.OFFSET, 7]
_CACHE = {}


def _np(x):
    return np.asarray(x.cpu() if hasattr(x, "cpu") else x)


def _model(pkg, damping=True, nsteps=500):
    model = pkg.RateStateModel(number_time_steps=nsteps)
    model.RadiationDamping = damping
    return model


def _data_rows(pkg, eng, dcs=(100.0, 1000.0)):
    """observations of the real model at nsteps 500 for the true Dc `dcs`, 1 % noise (tests/test_gpu_smc.py's recipe) → (G, nout)"""
    if dcs not in _CACHE:
        eng.set_model(_model(pkg), 1)
        truth = np.asarray(eng.forward(list(dcs))[1]).T
        rng = np.random.default_rng(1)
        _CACHE[dcs] = np.ascontiguousarray(truth + 0.01 * np.abs(truth).max(axis=1, keepdims=True) * rng.standard_normal(truth.shape))
    return _CACHE[dcs]


def _crafted(n):
    """l (3, n): the crafted spread with a tenth at -inf; one dominant particle among weights that underflow; all equal"""
    one = -50.0 + np.random.default_rng(2).standard_normal(n)
    one[n // 3] = 900.0
    one[5] = -np.inf
    return np.stack([cases.crafted_l(n), one, np.full(n, -3.25)])


# ---- 1. the stage kernels ---------------------------------------------------------------------------------------------------------
def _stage_results(eng, n):
    """every stage kernel's output for the crafted populations, as host arrays"""
    l = _crafted(n)
    rng = np.random.default_rng(n)
    q = rng.uniform(size=(P, n, 3))
    deltas = np.stack([np.array(cases.DELTAS), 0.5 * np.array(cases.DELTAS), np.linspace(0.0, 1.0, len(cases.DELTAS))])
    lmax = np.array([l[p][np.isfinite(l[p])].max() for p in range(P)])
    out = {"init1": eng.smc_batch_init(*cases.BOXES[1], n, SEEDS, OFFSETS), "init3": eng.smc_batch_init(*cases.BOXES[3], n, SEEDS, OFFSETS),
           "own": eng.smc_batch_weight_sums(l, deltas), "given": eng.smc_batch_weight_sums(l, deltas, lmax + [0.0, 1.5, -2.0]),
           "resample": eng.smc_batch_resample(q, l, [0.01, 1.0, 0.37], lmax, [0.37, 1.0, 2.0 ** -53]),
           "std2": eng.smc_batch_std2(np.where(np.isfinite(l), l, -40.0), 250.0, SEEDS, OFFSETS, [0, 19, 4])}
    out["resample"] = [_np(x) for x in out["resample"]]
    for key in ("init1", "init3", "std2"):
        out[key] = _np(out[key])
    return out, q, l, deltas, lmax


@pytest.mark.parametrize("n", [N, 2500])
def test_stage_kernels_bit_for_bit(pkg, gpu_engine, n):
    got, q, l, deltas, lmax = _stage_results(gpu_engine, n)
    for p in range(P):
        for d in (1, 3):
            np.testing.assert_array_equal(got[f"init{d}"][p], gpu_engine.smc_init(*cases.BOXES[d], n, SEEDS[p], OFFSETS[p]))
        for key, lm in (("own", None), ("given", float(lmax[p] + [0.0, 1.5, -2.0][p]))):
            want = gpu_engine.smc_weight_sums(l[p], deltas[p], lm)
            assert (got[key][p]["lmax"], got[key][p]["n_finite"], got[key][p]["n_neginf"]) == (want["lmax"], want["n_finite"], want["n_neginf"])
            np.testing.assert_array_equal(got[key][p]["sums"], want["sums"])
        want = gpu_engine.smc_resample(q[p], l[p], [0.01, 1.0, 0.37][p], lmax[p], [0.37, 1.0, 2.0 ** -53][p])
        for a, b in zip(got["resample"], want):
            np.testing.assert_array_equal(a[p], b)
        assert got["resample"][1][p].min() >= 0 and got["resample"][1][p].max() < n  # ancestors are local to the population
        np.testing.assert_array_equal(got["std2"][p], gpu_engine.smc_std2(np.where(np.isfinite(l[p]), l[p], -40.0), 250.0, SEEDS[p], OFFSETS[p], [0, 19, 4][p]))
    assert (got["resample"][1][1] == n // 3).all()  # the dominant particle takes every offspring
    # device memory: the same bits
    with pkg.Engine(mem="device") as dev:
        other = _stage_results(dev, n)[0]
    for key in ("init1", "init3", "std2"):
        np.testing.assert_array_equal(other[key], got[key])
    for a, b in zip(other["resample"], got["resample"]):
        np.testing.assert_array_equal(a, b)
    for key in ("own", "given"):
        for a, b in zip(other[key], got[key]):
            assert (a["lmax"], a["n_finite"], a["n_neginf"]) == (b["lmax"], b["n_finite"], b["n_neginf"])
            np.testing.assert_array_equal(a["sums"], b["sums"])


@pytest.mark.parametrize("mem", ["host", "device"])
def test_an_inactive_population_is_left_alone(pkg, mem):
    n = N
    l = _crafted(n)
    q = np.random.default_rng(7).uniform(size=(P, n, 3))
    lmax = np.array([l[p][np.isfinite(l[p])].max() for p in range(P)])
    act = [True, False, True]
    with pkg.Engine(mem=mem) as eng:
        # the inactive population's l is unusable (NaN) and its parameters are invalid: neither is looked at
        bad = l.copy()
        bad[1] = np.nan
        res = eng.smc_batch_weight_sums(bad, cases.DELTAS, None, act)
        assert res[1] is None
        for p in (0, 2):
            np.testing.assert_array_equal(res[p]["sums"], eng.smc_weight_sums(l[p], cases.DELTAS)["sums"])
        out = [np.full((P, n), -7.0), np.full((P, n), -7, dtype=np.int64), np.full((P, n, 3), -7.0), np.full((P, n), -7.0)]
        if mem == "device":
            import torch

            out = [torch.as_tensor(b).to(f"cuda:{eng.device}") for b in out]
        cum, anc, qo, lo_ = (_np(x) for x in eng.smc_batch_resample(q, bad, [0.01, -1.0, 0.37], [lmax[0], np.inf, lmax[2]], [0.37, 5.0, 1.0], act, out=out))
        assert (cum[1] == -7.0).all() and (anc[1] == -7).all()                                  # not touched
        np.testing.assert_array_equal(qo[1], q[1])                                                # copied through
        np.testing.assert_array_equal(lo_[1], bad[1])
        for p in (0, 2):
            want = eng.smc_resample(q[p], l[p], [0.01, -1.0, 0.37][p], lmax[p], [0.37, 5.0, 1.0][p])
            for a, b in zip((cum, anc, qo, lo_), want):
                np.testing.assert_array_equal(a[p], _np(b))


# ---- 2. the fused move ------------------------------------------------------------------------------------------------------------
def _move_case(eng, data, d, n, steps=3):
    lo, hi = np.array([600.0, 0.009, 0.013])[:d], np.array([1600.0, 0.013, 0.017])[:d]
    shape = 0.5 * data.shape[1]
    group = [0, 1, 0]
    q = _np(eng.smc_batch_init(lo, hi, n, SEEDS, OFFSETS))
    base = np.diag([120.0, 4e-4, 4e-4][:d]) + (np.array([[0, 0, 0], [-1e-4, 0, 0], [1e-5, -2e-5, 0]])[:d, :d])
    # population 2: a factor 1e9 times wider than the box — every proposal leaves it, no wave of that population solves
    chol = np.stack([base, 0.5 * base, np.diag(1e9 * (hi - lo))])
    return dict(lo=lo, hi=hi, shape=shape, group=group, q=q, chol=chol, beta=[0.37, 1.0, 0.05], iter0=[4, 1, 190], steps=steps)


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("d", [1, 3])
def test_fused_move_bit_for_bit(pkg, gpu_engine, d, damping):
    data = _data_rows(pkg, gpu_engine)
    gpu_engine.set_model(_model(pkg, damping), 1)
    c = _move_case(gpu_engine, data, d, N)
    l = gpu_engine.smc_batch_logtarget(c["q"], data, c["group"], c["lo"], c["hi"], c["shape"])
    for p in range(P):  # the start's l is the bridge sampler's with no transform and logg = 0
        np.testing.assert_array_equal(l[p], gpu_engine.evidence_logtarget(c["q"][p], data[c["group"][p]], c["lo"], c["hi"], np.zeros(N), c["shape"]))
    assert np.isfinite(l).all()
    args = (data, c["group"], c["lo"], c["hi"], c["chol"], c["beta"], SEEDS, OFFSETS, c["iter0"], c["steps"], c["shape"])
    q2, l2, acc = gpu_engine.smc_batch_move(c["q"], l, *args)
    singles = []
    for p in range(P):
        qs, ls, a = gpu_engine.smc_move(c["q"][p], l[p], data[c["group"][p]], c["lo"], c["hi"], c["chol"][p], c["beta"][p], SEEDS[p], OFFSETS[p],
                                        c["iter0"][p], c["steps"], c["shape"])
        singles.append((qs, ls, a))
        np.testing.assert_array_equal(q2[p], qs)
        np.testing.assert_array_equal(l2[p], ls)
        np.testing.assert_array_equal(acc[p], a)
    print(f"d {d} damping {damping}: accepted per population and step {acc.tolist()}")
    assert (acc[:2] > 0).all() and (acc[:2] < N).all()                         # the solving populations move ...
    assert (acc[2] == 0).all() and (q2[2] == c["q"][2]).all()                  # ... beside one whose waves never solve
    assert (q2[0] != c["q"][0]).any() and (q2[1] != c["q"][1]).any()
    # the two data rows matter: population 0 against the other row is another chain
    assert not np.array_equal(gpu_engine.smc_move(c["q"][0], l[0], data[1], c["lo"], c["hi"], c["chol"][0], c["beta"][0], SEEDS[0], OFFSETS[0],
                                                  c["iter0"][0], c["steps"], c["shape"])[1], singles[0][1])
    # an inactive population is not touched, whatever its parameters; the others are as before
    beta = [c["beta"][0], np.nan, c["beta"][2]]
    q3, l3, acc3 = gpu_engine.smc_batch_move(c["q"], l, data, [0, 99, 0], c["lo"], c["hi"], c["chol"] * np.array([1, 0, 1]).reshape(3, 1, 1), beta, SEEDS,
                                             OFFSETS, [4, 0, 190], c["steps"], c["shape"], active=[1, 0, 1])
    np.testing.assert_array_equal(q3[1], c["q"][1])
    np.testing.assert_array_equal(l3[1], l[1])
    assert (acc3[1] == 0).all()
    for p in (0, 2):
        np.testing.assert_array_equal(q3[p], q2[p])
        np.testing.assert_array_equal(l3[p], l2[p])
        np.testing.assert_array_equal(acc3[p], acc[p])
    # device memory: the same bits
    with pkg.Engine(mem="device") as dev:
        dev.set_model(_model(pkg, damping), 1)
        qd, ld, accd = dev.smc_batch_move(c["q"], l, *args)
        np.testing.assert_array_equal(_np(qd), q2)
        np.testing.assert_array_equal(_np(ld), l2)
        np.testing.assert_array_equal(accd, acc)


# ---- 3. the whole run -------------------------------------------------------------------------------------------------------------
def test_whole_run_equals_the_single_runs(pkg, gpu_engine):
    """2 groups x 2 replicates.  The two data rows (true Dc 100 and 1000 in the box (0, 1e4)) take different numbers of stages, so
    some populations go inactive while the others continue."""
    data = _data_rows(pkg, gpu_engine)
    gpu_engine.set_model(_model(pkg), 1)
    out = gpu_engine.smc_batch(data, [0.0], [1.0e4], N, replicates=2)
    runs = out["runs"]
    assert [(r["group"], r["replicate"], r["seed"]) for r in runs] == [(0, 0, 0), (0, 1, 1), (1, 0, 0), (1, 1, 1)]
    counts = []
    for r in runs:
        want = gpu_engine.smc(data[r["group"]], [0.0], [1.0e4], N, seed=r["seed"])
        counts.append(len(want["stages"]))
        assert r["stages"] == want["stages"]  # the ladder, each stage's delta, ess, accept rate and log I so far; the stage count
        for key in ("q", "l", "std2"):
            np.testing.assert_array_equal(r[key], want[key])
        assert (r["log_integral"], r["log_evidence"], r["n_solves"]) == (want["log_integral"], want["log_evidence"], want["n_solves"])
        assert r["stages"][-1]["beta"] == 1.0
    print(f"stage counts of the four populations: {counts}")
    assert len(set(counts)) > 1, counts  # otherwise no population went inactive before the others and the test proves nothing
    for g, s in enumerate(out["summary"]):
        le = np.array([r["log_evidence"] for r in runs if r["group"] == g])
        assert s["group"] == g and s["replicates"] == 2 and le.min() <= s["log_evidence_mean"] <= le.max()
        assert s["log_evidence_sd"] == pytest.approx(le.std(ddof=1)) and s["log_evidence_se"] > 0.0


def test_sample_smc_replicates(pkg, gpu_engine):
    data = _data_rows(pkg, gpu_engine)[1]
    m = pkg.MCMC(_model(pkg), data, 1000.0, ["Uniform", 0.0, 1.0e4], 1000.0, nsamples=10, verbose=False)
    one, three = m.sample_smc(N, seed=2), m.sample_smc(N, seed=2, replicates=3)
    np.testing.assert_array_equal(three.samples, one.samples)  # the first replicate is the run replicates = 1 gives
    np.testing.assert_array_equal(three.std2, one.std2)
    assert three.stats["log_evidence"] == one.stats["log_evidence"] == three.stats["replicate_log_evidence"][0]
    assert three.stats["replicate_log_evidence"].shape == (3,) and three.stats["log_evidence_se"] > 0.0
    assert "log_evidence_se" not in one.stats


# ---- 4. a table staged in more than one chunk -------------------------------------------------------------------------------------
def test_chunked_table(pkg, gpu_engine):
    """nsteps 800 with 4 RK4 steps per sample: 2 S kc + 1 loading values, kc observations and sample 0 must fit the sampler
    family's 56 KiB of LDS (csrc/rsf_kernel_common.h, rsf_set_model), kc = floor((7168 - 2) / 9) = 796 < nout - 1: two chunks.
    (796 x 9 is the largest table that fits, so nsteps 798 would be the smallest shape; 800 keeps the time step a round number.)"""
    S, n, dcs = 4, 130, (300.0, 1000.0)
    model = _model(pkg, True, 800)
    gpu_engine.set_model(model, S)
    kc = (56 * 1024 // 8 - 2) // (2 * S + 1)
    assert -(-(gpu_engine.nout - 1) // kc) == 2
    truth = np.asarray(gpu_engine.forward(list(dcs))[1]).T
    data = np.ascontiguousarray(truth + 0.01 * np.abs(truth).max() * np.random.default_rng(4).standard_normal(truth.shape))
    lo, hi, shape = [600.0], [1600.0], 0.5 * data.shape[1]
    seeds, offs, beta, it0 = [3, 4], [0, 11], [0.2, 0.9], [1, 7]
    q = gpu_engine.smc_batch_init(lo, hi, n, seeds, offs)
    l = gpu_engine.smc_batch_logtarget(q, data, [1, 0], lo, hi, shape)
    chol = np.array([[[90.0]], [[40.0]]])
    q2, l2, acc = gpu_engine.smc_batch_move(q, l, data, [1, 0], lo, hi, chol, beta, seeds, offs, it0, 3, shape)
    for p in range(2):
        row = data[[1, 0][p]]
        np.testing.assert_array_equal(l[p], gpu_engine.evidence_logtarget(q[p], row, lo, hi, np.zeros(n), shape))
        qs, ls, a = gpu_engine.smc_move(q[p], l[p], row, lo, hi, chol[p], beta[p], seeds[p], offs[p], it0[p], 3, shape)
        np.testing.assert_array_equal(q2[p], qs)
        np.testing.assert_array_equal(l2[p], ls)
        np.testing.assert_array_equal(acc[p], a)
    assert (acc > 0).all()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, gpu_engine):
    E = pkg.RsfError

    def code(fn, *a, **kw):
        with pytest.raises(E) as ei:
            fn(*a, **kw)
        return ei.value.code, str(ei.value)

    eng, n = gpu_engine, 10
    # P = 0 and P = 65, through the C ABI itself
    lib, dbl = eng.lib, ctypes.POINTER(ctypes.c_double)
    lo, hi, q = np.zeros(1), np.ones(1), np.zeros(65 * n)
    sd, off = np.zeros(65, dtype=np.uint64), np.zeros(65, dtype=np.int64)
    for bad_p in (0, 65):
        rc = lib.rsf_smc_batch_init(eng._ctx, bad_p, n, 1, lo.ctypes.data_as(dbl), hi.ctypes.data_as(dbl), sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                    off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), q.ctypes.data)
        assert rc == -1 and b"1 <= P <= 64" in lib.rsf_last_error()
    assert lib.rsf_smc_batch_init(eng._ctx, 2, n, 1, lo.ctypes.data_as(dbl), hi.ctypes.data_as(dbl), None,
                                  off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), q.ctypes.data) == -1  # a NULL array
    assert code(eng.smc_batch_init, [0.0], [1.0], n, np.arange(65))[0] == -1
    assert code(eng.smc_batch_init, [0.0], [1.0], 0, [1, 2])[0] == -1
    c, msg = code(eng.smc_batch_init, [0.0], [1.0], n, [1, 2, 3], [0, 0, -1])
    assert c == -1 and "population 2" in msg
    # a population with no finite l, one with a NaN: that population's error, by name
    l = np.zeros((3, n))
    l[1] = -np.inf
    c, msg = code(eng.smc_batch_weight_sums, l, [0.5])
    assert c == -1 and "population 1" in msg and "every particle has l = -inf" in msg
    assert eng.smc_batch_weight_sums(l, [0.5], None, [1, 0, 1])[1] is None  # ... and nobody's when it is inactive
    l[1] = 0.0
    l[2, 3] = np.nan
    c, msg = code(eng.smc_batch_weight_sums, l, [0.5])
    assert c == -1 and "population 2" in msg and "NaN" in msg
    c, msg = code(eng.smc_batch_weight_sums, np.zeros((3, n)), [[0.5], [0.5], [-0.5]])
    assert c == -1 and "population 2" in msg
    c, msg = code(eng.smc_batch_resample, np.zeros((3, n, 1)), np.zeros((3, n)), 0.5, 0.0, [0.5, 0.0, 0.5])
    assert c == -1 and "population 1" in msg
    # the move: no model, a bad group index, a bad factor, a DOP853 model
    qq, ll, ok = np.full((3, n, 1), 1000.0), np.zeros((3, n)), ([0.0], [1e4], np.ones((3, 1, 1)), 0.5, [1, 2, 3])
    with pytest.raises(E, match="set_model"):
        eng.smc_batch_move(qq, ll, np.zeros((2, 50)), [0, 1, 0], *ok)
    model = pkg.RateStateModel(number_time_steps=50)
    eng.set_model(model, 1)
    data = np.zeros((2, eng.nout))
    assert eng.smc_batch_move(qq, ll, data, [0, 1, 0], *ok)[0].shape == (3, n, 1)
    for grp in ([0, 2, 0], [0, -1, 0]):
        c, msg = code(eng.smc_batch_move, qq, ll, data, grp, *ok)
        assert c == -1 and "population 1" in msg and "group" in msg
    c, msg = code(eng.smc_batch_logtarget, qq, data, [0, 1, 2], [0.0], [1e4])
    assert c == -1 and "population 2" in msg
    c, msg = code(eng.smc_batch_move, qq, ll, data, 0, [0.0], [1e4], np.array([1.0, 1.0, 0.0]).reshape(3, 1, 1), 0.5, [1, 2, 3])
    assert c == -1 and "population 2" in msg and "chol" in msg
    c, msg = code(eng.smc_batch_move, qq, ll, data, 0, [0.0], [1e4], np.ones((3, 1, 1)), [0.5, 0.0, 0.5], [1, 2, 3])
    assert c == -1 and "population 1" in msg and "beta" in msg
    assert code(eng.smc_batch_move, qq, ll, data, 0, *ok, steps=65)[0] == -1
    assert code(eng.smc_batch_move, np.ones((3, n, 2)), ll, data, 0, [0.0, 0.0], [1.0, 1.0], np.tile(np.eye(2), (3, 1, 1)), 0.5, [1, 2, 3])[0] == -1
    assert code(eng.smc_batch_std2, ll, 0.5, [1, 2, 3])[0] == -1
    model.integrator = "dop853"
    eng.set_model(model, 1)
    c, msg = code(eng.smc_batch_move, qq, ll, data, [0, 1, 0], *ok)
    assert c == -5 and "DOP853" in msg
    assert code(eng.smc_batch_logtarget, qq, data, 0, [0.0], [1e4])[0] == -5
    assert "DOP853" in code(eng.smc_batch, data, [0.0], [1e4], n, replicates=2)[1]
