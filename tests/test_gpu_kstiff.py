"""
GPU tests of the delayed-rejection sampler with the stiffness of the apparatus among the parameters (include/rsf_kstiff.h:
rsf_kstiff_observe / _dr_run / _dr_ssq / _dr_propose / _dr_accept; Engine.kstiff_*, MCMC.sample_stiffness):
  1. rsf_kstiff_observe against rsf_stiff_observe, SSq and series bit for bit, with one k on every lane and with k varying;
  2. rsf_kstiff_dr_ssq on a mask that empties a whole wave, against rsf_kstiff_observe on the compacted points, bit for bit;
  3. rsf_kstiff_dr_propose / _accept at d = 2 are rsf_dr_propose / rsf_dr_accept bit for bit;
  4. the d = 4 chain logic keeps a closed-form target (no solve in the loop);
  5. the fused kernel against the split path, bit for bit;
  6. the target at d = 2 against the quadrature yardstick, whose SSq is the parent's kernel's;
  7. the target at d = 4 against the importance-sampling yardstick of the CPU specification;
  8. the front end and the C ABI's refusals.
Shapes: law_cases.spec() (nsteps 500) unless the matrix entry says otherwise; 12 lanes, 70, 133; 128 and 256 chains.
"""
import functools

import numpy as np
import pytest

import dr_cases
import kstiff_cases as KC
import kstiff_reference as KR
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
K_RANGE = (1e-3, 1e-2)  # the stiffness's box in the bit-identity tests
BOX = {2: (np.array([LS.LO3[0], K_RANGE[0]]), np.array([LS.HI3[0], K_RANGE[1]])),
       4: (np.append(LS.LO3, K_RANGE[0]), np.append(LS.HI3, K_RANGE[1]))}
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


def _noisy(clean, seed):
    return clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(seed).standard_normal(clean.size)


def _counters(n):
    return [np.zeros(n, dtype=np.int32) for _ in COUNTERS]


# ---- 1. rsf_kstiff_observe is rsf_stiff_observe ---------------------------------------------------------------------------------------------
def _entry(name):
    if name == "chunks_ab":
        return M.config(name)[0]
    return C.spec() if name == "damped" else C.spec(k1=0.0)


@pytest.mark.parametrize("name", ["damped", "k1zero", "chunks_ab"])
@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("law", R.LAWS)
def test_observe_with_one_stiffness_is_stiff_observe(pkg, gpu_engine, law, history, name):
    """k = 4e-3 on every lane, per-lane (a, b): series and SSq of all four observables are rsf_stiff_observe's bit for bit, 12 lanes
    and 70 — damped, with k1 = 0, and with the table in two chunks (nsteps 900, substeps 4)."""
    m = _entry(name)
    eng = gpu_engine
    eng.set_model(_model(pkg, m, R.table(m, history)), m.substeps)
    a12, b12 = M.lane_ab()
    for idx in (np.arange(12), SC.lanes70()):
        dc, a, b = np.asarray(R.LANES)[idx], np.ascontiguousarray(a12[idx]), np.ascontiguousarray(b12[idx])
        k = np.full(idx.size, SC.K_ACC)
        for obs in O.OBSERVABLES:
            want = np.asarray(eng.stiff_observe(law, obs, SC.K_ACC, dc, a, b)[1])
            data = _noisy(want[:, 3], 4)
            want_ssq = eng.stiff_observe(law, obs, SC.K_ACC, dc, a, b, data=data, want_ssq=True, want_series=False)[0]
            ssq, got = eng.kstiff_observe(law, obs, dc, k, a, b, data=data, want_ssq=True, want_series=True)
            assert np.isfinite(want).all() and np.isfinite(want_ssq).all() and np.abs(want - want[0]).max() > 0, obs
            assert np.array_equal(_bits(got), _bits(want)), (obs, idx.size)
            assert np.array_equal(_bits(ssq), _bits(want_ssq)), (obs, idx.size)
            # SSq alone, and the model's (a, b) where none are given
            only = eng.kstiff_observe(law, obs, dc, k, a, b, data=data, want_ssq=True, want_series=False)[0]
            assert np.array_equal(_bits(only), _bits(want_ssq)), obs
        plain = eng.kstiff_observe(law, "mu", dc, k)[1]
        assert np.array_equal(_bits(plain), _bits(eng.stiff_observe(law, "mu", SC.K_ACC, dc)[1]))


@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("law", R.LAWS)
def test_observe_with_a_stiffness_per_lane(pkg, gpu_engine, law, history):
    """k from 3e-3 to 8e-3 over the lanes: each lane's series and SSq are those of an rsf_stiff_observe call with that lane's k — 12
    lanes and 70, whatever the lane's neighbours carry; and the model's own stiffness plays no part."""
    m = C.spec()
    eng = gpu_engine
    a12, b12 = M.lane_ab()
    k12 = np.linspace(3e-3, 8e-3, 12)[np.random.default_rng(2).permutation(12)]
    for stiffness in (None, 1.7e-3):
        eng.set_model(_model(pkg, m, R.table(m, history), stiffness=stiffness), 1)
        for idx in (np.arange(12), SC.lanes70()):
            dc, a, b, k = (np.ascontiguousarray(x[idx]) for x in (np.asarray(R.LANES), a12, b12, k12))
            for obs in O.OBSERVABLES:
                got = np.asarray(eng.kstiff_observe(law, obs, dc, k, a, b)[1])
                data = _noisy(got[:, 3], 4)
                ssq = np.asarray(eng.kstiff_observe(law, obs, dc, k, a, b, data=data, want_ssq=True, want_series=False)[0])
                assert np.isfinite(got).all() and np.isfinite(ssq).all(), obs
                for i in range(12):  # the twelve distinct lanes; a tiled lane repeats its first copy
                    one_ssq, one = eng.stiff_observe(law, obs, float(k12[i]), [R.LANES[i]], [a12[i]], [b12[i]], data=data, want_ssq=True)
                    for j in np.flatnonzero(idx == i):
                        assert np.array_equal(_bits(got[:, j]), _bits(np.asarray(one)[:, 0])), (obs, i, j)
                        assert _bits(ssq[j]) == _bits(np.asarray(one_ssq)[0]), (obs, i, j)
            if stiffness is not None:
                break  # once more on 12 lanes with a stiffness of the model's: the same bits as an explicit call


# ---- 2. one stage's SSq --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dr_data(law, obs):
    """two observation series of the constant-k model at the truth (20, 0.011, 0.014), k = 4e-3, step history: two noise draws"""
    m = C.spec()
    clean = S.forward(m, SC.K_ACC, [R.BF_TRUTH], R.table(m, "step"), law, obs)[0][:, 0]
    return np.stack([_noisy(clean, R.BF_SEED), _noisy(clean, R.BF_SEED + 1)])


def _observe_ssq(eng, law, obs, y, mask, data):
    """rsf_kstiff_observe's SSq of the masked-in proposals, group by group against the group's series -> (n,), 1 elsewhere"""
    y, mask = np.asarray(y), np.asarray(mask)
    G = data.shape[0]
    per, out = y.shape[0] // G, np.ones(y.shape[0])
    for g in range(G):
        rows = np.flatnonzero(mask[g * per:(g + 1) * per]) + g * per
        if rows.size:
            dc, a, b, k = (None if x is None else np.ascontiguousarray(x) for x in KR.columns(y[rows]))
            out[rows] = eng.kstiff_observe(law, obs, dc, k, a, b, data=data[g], want_ssq=True, want_series=False)[0]
    return out


@pytest.mark.parametrize("d", [2, 4])
def test_stage_ssq_is_kstiff_observe_bit_for_bit(pkg, d):
    """rsf_kstiff_dr_ssq on 133 lanes whose mask empties a whole wave (lanes 64 .. 127) against rsf_kstiff_observe on the compacted
    points; untouched entries keep their sentinel; and with one k on every lane it is rsf_stiff_dr_ssq's SSq too."""
    m = C.spec()
    n = 133
    lo, hi = BOX[d]
    with pkg.Engine(mem="host") as eng:
        eng.set_model(_model(pkg, m, R.table(m, "step")), 1)
        for law in R.LAWS:
            for obs in ("mu", "acc"):
                data = _dr_data(law, obs)[0]
                y = np.ascontiguousarray(lo + (hi - lo) * np.random.default_rng([n, d]).uniform(0.2, 0.95, (n, d)))
                mask = ((np.arange(n) % 3 != 2) & ~((np.arange(n) >= 64) & (np.arange(n) < 128))).astype(np.uint8)
                got = np.asarray(eng.kstiff_dr_ssq(law, obs, y, mask, data, ssq=np.full(n, SENT)))
                want = _observe_ssq(eng, law, obs, y, mask, data[None])
                rows = mask == 1
                assert rows.sum() > 40 and np.isfinite(want[rows]).all() and np.array_equal(_bits(got[rows]), _bits(want[rows])), (law, obs)
                assert (got[~rows] == SENT).all(), (law, obs)
                same = y.copy()
                same[:, -1] = SC.K_ACC
                ones = np.ones(n, dtype=np.uint8)
                stiff = np.asarray(eng.stiff_dr_ssq(law, obs, SC.K_ACC, np.ascontiguousarray(same[:, :-1]), ones, data))
                assert np.isfinite(stiff).all() and np.array_equal(_bits(eng.kstiff_dr_ssq(law, obs, same, ones, data)), _bits(stiff)), (law, obs)


# ---- 3. the split pair at d = 2 --------------------------------------------------------------------------------------------------------------
def test_split_pair_at_two_parameters_is_the_parent_pair(gpu_engine):
    """dr_cases.split_problem(2) — 257 chains and rows crafted for every way an iteration ends, its second box in k > 0 — through
    rsf_kstiff_dr_propose / _accept and through rsf_dr_propose / rsf_dr_accept: proposals, masks, l1, pending, states and all five
    counters bit for bit, both stages of every iteration."""
    eng = gpu_engine
    prob = dr_cases.split_problem(2)
    lo, hi, L, shape = prob["lo"], prob["hi"], prob["L"], prob["shape"]
    assert lo[1] > 0
    q0 = prob["q0"]
    with np.errstate(all="ignore"):
        l0 = -shape * np.log(prob["fn"](q0))
    for row, v in prob["bad_l"].items():
        l0[row] = v
    n = q0.shape[0]
    new, old = [dict(q=q0.copy(), l=l0.copy(), c=_counters(n)) for _ in range(2)]
    calls = ((new, eng.kstiff_dr_propose, eng.kstiff_dr_accept), (old, eng.dr_propose, eng.dr_accept))
    for it in range(1, dr_cases.SPLIT_ITERS + 1):
        kw = dict(gamma=dr_cases.SPLIT_GAMMA, seed=dr_cases.SPLIT_SEED, offset=dr_cases.SPLIT_OFFSET, iteration=it)
        out = []
        for st, propose, accept in calls:
            y1, m1 = propose(st["q"], st["l"], lo, hi, L, 1, **kw)
            s1 = prob["fix"](1, np.where(np.asarray(m1) == 1, prob["fn"](np.asarray(y1)), 1.0))
            l1, pend = accept(st["q"], st["l"], lo, hi, 1, y1, m1, s1, st["c"], shape, **kw)
            y2, m2 = propose(st["q"], st["l"], lo, hi, L, 2, pending=pend, **kw)
            s2 = prob["fix"](2, np.where(np.asarray(m2) == 1, prob["fn"](np.asarray(y2)), 1.0))
            accept(st["q"], st["l"], lo, hi, 2, y2, m2, s2, st["c"], shape, l1=l1, pending=pend, **kw)
            out.append((y1, m1, l1, pend, y2, m2, st["q"].copy(), st["l"].copy(), *[c.copy() for c in st["c"]]))
        for name, a, b in zip(("y1", "mask1", "l1", "pending", "y2", "mask2", "q", "l") + COUNTERS, *out):
            assert np.array_equal(_bits(a), _bits(b)), (it, name)
    a1, a2, o1, o2, stuck = new["c"]
    print(f"d 2 split pair: counters { {k: int(v.sum()) for k, v in zip(COUNTERS, new['c'])} } of {dr_cases.SPLIT_ITERS * n}")
    assert a1.sum() > 0 and a2.sum() > 0 and o1.sum() > 0 and o2.sum() > 0 and stuck.sum() == 3 * dr_cases.SPLIT_ITERS


# ---- 4. the chain logic at d = 4 on a closed form ----------------------------------------------------------------------------------------------
def test_chain_logic_keeps_the_closed_form_at_four_parameters(gpu_engine):
    """kstiff_cases.CLOSED4, dr_cases' quadratic SSq widened to four parameters: 262 144 chains drawn from the exact target are advanced
    by rsf_kstiff_dr_propose -> the closed form on the host -> rsf_kstiff_dr_accept, two stages per iteration, and held to the target
    after iterations 4 and 8 by tests/test_gpu_dr.py's rule: per parameter and for sigma^2 the mean and the variance within Z_MAX = 4.5
    standard errors and sqrt(C) x the KS distance below KS_MAX = 2.4."""
    eng = gpu_engine
    ref, c = KC.closed4(), KC.CLOSED4
    scale, gamma = KC.LEG4
    n, shape = KC.C_TARGET, c["shape"]
    fn = dr_cases.rows_fn(ref.fn, 4)
    q = ref.draw(np.random.default_rng([KC.SEED4, 4]), n)
    l = -shape * np.log(fn(q))
    L = KC.closed4_factor(scale)
    cnt = _counters(n)
    solved = lambda y, mask: np.where(np.asarray(mask) == 1, fn(np.asarray(y)), 1.0)
    fails, zmax, kmax = [], 0.0, 0.0
    for it in range(1, max(KC.CHECKPOINTS) + 1):
        kw = dict(gamma=gamma, seed=KC.SEED4, offset=0, iteration=it)
        y, mask = eng.kstiff_dr_propose(q, l, c["lo"], c["hi"], L, 1, **kw)
        l1, pend = eng.kstiff_dr_accept(q, l, c["lo"], c["hi"], 1, y, mask, solved(y, mask), cnt, shape, **kw)
        y, mask = eng.kstiff_dr_propose(q, l, c["lo"], c["hi"], L, 2, pending=pend, **kw)
        eng.kstiff_dr_accept(q, l, c["lo"], c["hi"], 2, y, mask, solved(y, mask), cnt, shape, l1=l1, pending=pend, **kw)
        if it in KC.CHECKPOINTS:
            std2 = np.asarray(eng.smc_std2(l, shape, KC.SEED4, 0, it))
            z, k = KC.check4(f"closed d 4 iteration {it}", ref, q, std2, fails)
            zmax, kmax = max(zmax, z), max(kmax, k)
    a1, a2, o1, o2, stuck = (int(x.sum()) for x in cnt)
    total = max(KC.CHECKPOINTS) * n
    print(f"closed d 4: largest |z| {zmax:.2f}, sqrt(C) D {kmax:.2f}; accepted {a1 / total:.3f} + {a2 / total:.3f}, outside the box "
          f"{o1 / total:.3f} / {o2 / total:.3f}")
    assert stuck == 0 and a1 > 0 and a2 > 0 and o1 > 0 and o2 > 0
    assert not fails, fails


# ---- 5. fused = split ------------------------------------------------------------------------------------------------------------------------
def _starts(d, n):
    rng = np.random.default_rng(7)
    q = np.column_stack([rng.uniform(15.0, 25.0, n), rng.uniform(0.0105, 0.0115, n), rng.uniform(0.0135, 0.0145, n), rng.uniform(3e-3, 5e-3, n)])
    return np.ascontiguousarray(q if d == 4 else q[:, [0, 3]])


@pytest.mark.parametrize("obs", ["mu", "acc"])
@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("d", [2, 4])
def test_fused_against_split(pkg, d, law, obs):
    """rsf_kstiff_dr_run against rsf_kstiff_dr_propose -> rsf_kstiff_observe -> rsf_kstiff_dr_accept: the state after every iteration
    and all five counters, bit for bit; one and two stages, two observation groups with two factors, 128 chains x 8 iterations in two
    launches of four, workgroups of 64.  With one stage accepted2 stays zero everywhere."""
    n, G = 128, 2
    m = C.spec()
    data = _dr_data(law, obs)
    lo, hi = BOX[d]
    shape = 0.5 * data.shape[-1]
    q0 = _starts(d, n)
    per = n // G
    truth = np.append(LS.TRUTH3, SC.K_ACC) if d == 4 else np.array([LS.TRUTH3[0], SC.K_ACC])
    with pkg.Engine(mem="host", block_threads=64) as eng:
        eng.set_model(_model(pkg, m, R.table(m, "step")), 1)
        # the friction series' Gauss-Newton factor under either observable: the acceleration hardly determines four parameters, and its
        # own factor at d = 4 sends every first proposal out of the box
        L1 = eng.kstiff_gn_factor(law, "mu", truth, _dr_data(law, "mu")[0])[0]
        L = np.stack([L1, 2.0 * L1])
        l0 = np.concatenate([-shape * np.log(eng.kstiff_ssq_fn(law, data[g], obs)(q0[g * per:(g + 1) * per])) for g in range(G)])
        assert np.isfinite(l0).all()
        for stages in (1, 2):
            fused, split = [dict(q=q0.copy(), l=l0.copy(), c=_counters(n)) for _ in range(2)]
            for first in (1, 5):
                tq, tl = eng.kstiff_dr_run(law, obs, fused["q"], fused["l"], data, lo, hi, L, 4, fused["c"], gamma=GAMMA, stages=stages, shape=shape,
                                           seed=SEED, offset=OFFSET, iter0=first, trace=True)
                for j, it in enumerate(range(first, first + 4)):
                    kw = dict(gamma=GAMMA, seed=SEED, offset=OFFSET, iteration=it)
                    y, mk = eng.kstiff_dr_propose(split["q"], split["l"], lo, hi, L, 1, **kw)
                    l1, pend = eng.kstiff_dr_accept(split["q"], split["l"], lo, hi, 1, y, mk, _observe_ssq(eng, law, obs, y, mk, data), split["c"], shape, **kw)
                    if stages == 2:
                        y, mk = eng.kstiff_dr_propose(split["q"], split["l"], lo, hi, L, 2, pending=pend, **kw)
                        eng.kstiff_dr_accept(split["q"], split["l"], lo, hi, 2, y, mk, _observe_ssq(eng, law, obs, y, mk, data), split["c"], shape, l1=l1,
                                             pending=pend, **kw)
                    assert np.asarray(tq)[j].tobytes() == split["q"].tobytes() and np.asarray(tl)[j].tobytes() == split["l"].tobytes(), (stages, it)
                same = {key: bool(np.array_equal(_bits(fused[key]), _bits(split[key]))) for key in ("q", "l")}
                same.update({key: bool(np.array_equal(a, b)) for key, a, b in zip(COUNTERS, fused["c"], split["c"])})
                print(f"d {d} {law} {obs} stages {stages} after iteration {first + 3}: counters "
                      f"{ {key: int(v.sum()) for key, v in zip(COUNTERS, fused['c'])} } of {(first + 3) * n}; bit-identical {same}")
                assert all(same.values()), same
            a1, a2, o1, o2, stuck = fused["c"]
            assert a1.sum() > 0 and (a2.sum() > 0) == (stages == 2) and stuck.sum() == 0 and (a1 + a2 <= 8).all()
            if stages == 1:
                assert (a2 == 0).all() and (o2 == 0).all()
            assert (fused["q"][:, -1] != q0[:, -1]).any()  # the stiffness moves


# ---- 6. the target at d = 2 --------------------------------------------------------------------------------------------------------------------
def _chain_means(x):
    """kept states (n_keep, n_chains) -> (mean of the per-chain means, its standard error)"""
    means = x.mean(axis=0)
    return float(means.mean()), float(means.std(ddof=1) / np.sqrt(means.size))


def test_sample_stiffness_keeps_the_quadrature_posterior(pkg):
    """Friction data from Dc = 20, k = 2e-3 under the hold history: MCMC.sample_stiffness at 256 chains x 400 iterations over
    (Dc, k) against the tensor Simpson quadrature whose SSq is rsf_stiff_observe's, one call per k node — the parent's kernel.  By
    tests/test_gpu_law_dr.py's rule the mean of the per-chain means lies within 4.5 standard errors of the quadrature's, for Dc and
    for k; no chain is stuck and the acceptance rate lies in (0.05, 0.95)."""
    p = KC.problem2("hold")
    model = _model(pkg, p["m"], p["vl"], observable="mu", stiffness=SC.K_WHY)
    with pkg.Engine(mem="host") as eng:
        eng.set_model(_model(pkg, p["m"], p["vl"], observable="mu"), 1)

        def parent_ssq(pts):
            out = np.empty(len(pts))
            for k in np.unique(pts[:, 1]):
                rows = pts[:, 1] == k
                out[rows] = eng.stiff_observe("aging", "mu", float(k), np.ascontiguousarray(pts[rows, 0]), data=p["data"], want_ssq=True, want_series=False)[0]
            return out

        coarse, exact = KC.yardstick2("hold", parent_ssq, n=(65, 33)), KC.yardstick2("hold", parent_ssq)
    assert (np.abs(coarse["mean"] / exact["mean"] - 1.0) < 1e-6).all() and exact["edge"] <= 1e-4
    mc = pkg.MCMC(model, p["data"], R.BF_TRUTH, ["Uniform", *R.BF_BOX], R.BF_TRUTH, nsamples=10, verbose=False)
    pool = mc.sample_stiffness(256, 400, KC.K_BOX, seed=9)
    x = np.asarray(pool.samples)
    assert x.shape == (200, 256, 2) and pool.stats["stuck"] == 0 and pool.stats["path"] == "kstiff_dr" and pool.stats["adapt"] is True
    assert np.asarray(pool.std2).shape == (200, 256) and np.isfinite(x).all()
    zs = []
    for j, name in enumerate(("Dc", "k")):
        mean, se = _chain_means(x[:, :, j])
        zs.append((mean - exact["mean"][j]) / se)
        print(f"{name}: pooled mean {mean:.6g}, quadrature {exact['mean'][j]:.6g} (SD {exact['sd'][j]:.3g}), pooled SD {x[:, :, j].std():.3g}, "
              f"SE {se:.2e}, z {zs[-1]:+.2f}")
    print(f"accept rate {pool.accept_rate:.2f}; quadrature 65 x 33 against 129 x 65 {np.abs(coarse['mean'] / exact['mean'] - 1.0)}, edge {exact['edge']:.1e}")
    assert 0.05 < pool.accept_rate < 0.95
    assert all(abs(z) < 4.5 for z in zs), zs


# ---- 7. the target at d = 4 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", R.LAWS)
def test_sample_stiffness_keeps_the_importance_posterior(pkg, law):
    """Friction data of the same recipe under the step history and `law`: MCMC.sample_stiffness at 256 chains x 800 iterations
    (nburn 400) over (Dc, a, b, k) against the self-normalised importance-sampling yardstick of the CPU specification (16 384 draws of
    a t5) — for each parameter |z| < 4.5 with the two standard errors combined; the yardstick's three conditions hold."""
    p = KC.problem4(law)
    y = p["yard"]
    assert y["inbox"] and y["finite"] and y["ess"] >= 0.25 * KC.IS_N and y["wmax"] <= 1e-3
    model = _model(pkg, p["m"], p["vl"], observable="mu", state_law=law, stiffness=SC.K_WHY)
    priors = [["Uniform", float(p["lo"][j]), float(p["hi"][j])] for j in range(3)]
    start = KC.truth(p["m"], 4)[:3]
    mc = pkg.MCMC(model, p["data"], R.BF_TRUTH, priors, start, nsamples=10, verbose=False)
    pool = mc.sample_stiffness(256, 800, (float(p["lo"][3]), float(p["hi"][3])), nburn=400, seed=9)
    x = np.asarray(pool.samples)
    assert x.shape == (400, 256, 4) and pool.stats["stuck"] == 0 and pool.stats["path"] == "kstiff_dr"
    zs = []
    for j, name in enumerate(("Dc", "a", "b", "k")):
        mean, se = _chain_means(x[:, :, j])
        zs.append((mean - y["mean"][j]) / np.hypot(se, y["se"][j]))
        print(f"{law} {name}: pooled mean {mean:.6g}, yardstick {y['mean'][j]:.6g} (SD {y['sd'][j]:.3g}, SE {y['se'][j]:.2e}), pooled SD "
              f"{x[:, :, j].std():.3g}, SE {se:.2e}, z {zs[-1]:+.2f}")
    print(f"{law}: accept rate {pool.accept_rate:.2f}; yardstick ESS / n {y['ess'] / KC.IS_N:.3f}, largest weight {y['wmax']:.2e}")
    assert 0.05 < pool.accept_rate < 0.95
    assert all(abs(z) < 4.5 for z in zs), zs


# ---- 8. the front end and the refusals of the C ABI ----------------------------------------------------------------------------------------------
def test_front_end(pkg, gpu_engine):
    """Engine.kstiff_dr is kstiff_dr_run launch by launch; kstiff_gn_factor is the specification's factor; kstiff_ssq_fn is
    kstiff_observe's SSq; a start outside the box or on a point without a finite SSq is refused."""
    m = C.spec()
    eng = gpu_engine
    eng.set_model(_model(pkg, m, R.table(m, "step")), 1)
    law, obs, d, n = "slip", "mu", 4, 64
    data = _dr_data(law, obs)[0]
    lo, hi = BOX[d]
    truth = np.append(LS.TRUTH3, SC.K_ACC)
    L, cov, ssq = eng.kstiff_gn_factor(law, obs, truth, data)
    Lw, covw, ssqw = KR.gn_factor(m, R.table(m, "step"), law, obs, truth, data)
    # the series agree to ~1e-12 of their excursion, a forward difference over a step of 1e-4 to ~1e-8, the inverse of J^T J (condition
    # number ~1e2) to ~1e-6: held to 1e-4
    assert abs(ssq / ssqw - 1.0) < 1e-9 and np.allclose(L, Lw, rtol=1e-4, atol=0.0) and np.allclose(cov, covw, rtol=1e-4, atol=0.0)
    q0 = _starts(d, n)
    s0 = eng.kstiff_ssq_fn(law, data, obs)(q0)
    want = KR.ssq_fn(m, R.table(m, "step"), law, obs, data)(q0)
    assert (np.abs(s0 - want) <= 1e-9 * want).all()
    res = eng.kstiff_dr(law, obs, q0, data, lo, hi, L, 8, gamma=GAMMA, seed=SEED, offset=OFFSET, iters_per_launch=4)
    q, l, cnt = q0.copy(), -0.5 * eng.nout * np.log(s0), _counters(n)
    for first in (1, 5):
        eng.kstiff_dr_run(law, obs, q, l, data, lo, hi, L, 4, cnt, gamma=GAMMA, seed=SEED, offset=OFFSET, iter0=first)
    assert np.array_equal(_bits(res.q), _bits(q)) and np.array_equal(_bits(res.l), _bits(l)) and res.trace_q.shape == (8, n, 4)
    assert all(np.array_equal(a, b) for a, b in zip((res.accepted1, res.accepted2, res.outbox1, res.outbox2, res.stuck), cnt))
    bad = q0.copy()
    bad[3, 3] = 2.0 * K_RANGE[1]
    with pytest.raises(ValueError, match="stuck start"):
        eng.kstiff_dr(law, obs, bad, data, lo, hi, L, 4)
    low = np.tile([6.0, 1e-3], (n, 1))  # below the critical stiffness: the slip-law trajectory is not finite (stiff_cases.K_LOW)
    assert not np.isfinite(eng.kstiff_ssq_fn(law, data, obs)(low)).any()
    with pytest.raises(ValueError, match="stuck start"):
        eng.kstiff_dr(law, obs, low, data, [5.0, 5e-4], [60.0, 1e-2], np.diag([1.0, 1e-5]), 4)


def test_refusals(pkg, gpu_engine):
    """RSF_ERR_INVALID naming the function: d not 2 or 4, lo[d - 1] <= 0, a k[i] that is not finite and > 0 (host and device
    callers); RSF_FLAG_DOP853: RSF_ERR_UNSUPPORTED; RSF_FLAG_FP32_SOLVE runs the float64 solve."""
    eng = gpu_engine
    m = C.spec()
    eng.set_model(_model(pkg, m, R.table(m, "step")), 1)
    data = _dr_data("aging", "mu")[0]
    n = 64
    ones = np.ones(n, np.uint8)
    for d, name_d in ((1, "need d = 2 or 4"), (3, "need d = 2 or 4")):
        q, l, cnt = np.full((n, d), 20.0), np.zeros(n), _counters(n)
        lo, hi, L = [5.0] * d, [200.0] * d, np.eye(d)
        for name, call in (("rsf_kstiff_dr_run", lambda: eng.kstiff_dr_run("aging", "mu", q, l, data, lo, hi, L, 1, cnt)),
                           ("rsf_kstiff_dr_ssq", lambda: eng.kstiff_dr_ssq("aging", "mu", q, ones, data)),
                           ("rsf_kstiff_dr_propose", lambda: eng.kstiff_dr_propose(q, l, lo, hi, L, 1)),
                           ("rsf_kstiff_dr_accept", lambda: eng.kstiff_dr_accept(q, l, lo, hi, 1, q, ones, np.ones(n), cnt, 25.0))):
            with pytest.raises(pkg.RsfError, match=f"{name}: {name_d}") as ei:
                call()
            assert ei.value.code == -1
    for d in (2, 4):
        q, l, cnt = np.ascontiguousarray(np.tile(([20.0, 0.011, 0.014, 4e-3] if d == 4 else [20.0, 4e-3]), (n, 1))), np.zeros(n), _counters(n)
        hi, L = BOX[d][1], np.diag([1.0, 1e-4, 1e-4, 1e-4][:d])
        for bad in (0.0, -1e-3):
            lo = BOX[d][0].copy()
            lo[-1] = bad
            for name, call in (("rsf_kstiff_dr_run", lambda: eng.kstiff_dr_run("aging", "mu", q, l, data, lo, hi, L, 1, cnt)),
                               ("rsf_kstiff_dr_propose", lambda: eng.kstiff_dr_propose(q, l, lo, hi, L, 1)),
                               ("rsf_kstiff_dr_accept", lambda: eng.kstiff_dr_accept(q, l, lo, hi, 1, q, ones, np.ones(n), cnt, 25.0))):
                with pytest.raises(pkg.RsfError, match=rf"{name}: need lo\[{d - 1}\] > 0") as ei:
                    call()
                assert ei.value.code == -1
    with pkg.Engine(mem="device") as dev:
        dev.set_model(_model(pkg, m, R.table(m, "step")), 1)
        for e in (eng, dev):
            for bad in (0.0, -4e-3, float("inf"), float("nan")):
                with pytest.raises(pkg.RsfError, match=r"rsf_kstiff_observe: k\[1\] must be finite and > 0") as ei:
                    e.kstiff_observe("aging", "mu", [20.0, 30.0, 40.0], [4e-3, bad, 4e-3])
                assert ei.value.code == -1
            good = np.asarray(_host(e.kstiff_observe("aging", "mu", [20.0, 30.0, 40.0], [4e-3, 5e-3, 4e-3])[1]))
            assert np.isfinite(good).all()
    with pytest.raises(pkg.RsfError, match="rsf_kstiff_observe: law is RSF_LAW_AGEING"):
        eng.kstiff_observe(7, 1, [20.0], [4e-3])
    plain = pkg.RateStateModel(number_time_steps=500)  # the built-in history
    eng.set_model(plain, 1)
    want = np.asarray(eng.kstiff_observe("aging", "mu", [20.0, 35.0], [4e-3, 5e-3])[1])
    assert np.isfinite(want).all()
    plain.precision = "float32"
    eng.set_model(plain, 1)
    assert np.array_equal(_bits(eng.kstiff_observe("aging", "mu", [20.0, 35.0], [4e-3, 5e-3])[1]), _bits(want))
    plain.precision, plain.integrator = "float64", "dop853"
    eng.set_model(plain, 1)
    q, l, cnt = np.ascontiguousarray(np.tile([20.0, 4e-3], (n, 1))), np.zeros(n), _counters(n)
    for call in (lambda: eng.kstiff_observe("aging", "mu", [20.0], [4e-3]),
                 lambda: eng.kstiff_dr_run("aging", "mu", q, l, data, *BOX[2], np.diag([1.0, 1e-4]), 1, cnt),
                 lambda: eng.kstiff_dr_ssq("aging", "mu", q, ones, data)):
        with pytest.raises(pkg.RsfError, match="RSF_FLAG_DOP853 is not supported") as ei:
            call()
        assert ei.value.code == -5


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x
