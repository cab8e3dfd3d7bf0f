"""
GPU tests of the affine-invariant ensemble sampler in islands (include/rsf_ensemble.h: rsf_ensemble_run / _propose / _accept;
Engine.ensemble*, MCMC.sample_ensemble) against the NumPy specification tests/ensemble_reference.py.

1. the split path against the specification, half-step by half-step from the GPU's own state: without log coordinates the proposal
   bit for bit (the one fused multiply-add is formed exactly in the specification); with them within 8 x the distance between
   NumPy's and the device's exp(log(.)) measured on the proposals themselves (the kernel's own exp and log, reached through a
   walker whose partner holds its own position: u' = v, q' = exp(log y)); every flag, counter and decision equal outside the tie
   band |log alpha - log U_a| <= 1e-9;
2. the fused kernel against the split path on the real model, bit for bit: the split path's SSq is rsf_ensemble_ssq's, the fused
   kernel's solve in its own arrangement (the tier code decides per wave, so rsf_fit_normal's SSq, whose waves hold other
   trajectories, agrees to rounding only: it is held to 1e-9, tier 1's bound);
3. island identity: an island run alone with its offset gives its rows of the full run, at every workgroup size;
4. targets: started in pi the walkers stay in pi — the island-level statistic (ensemble_reference.island_z) against the quadrature
   of posterior_reference, |z| < 4.5; the pooled check() is printed and asserted where ensemble_cases.POOLED_ASSERTED says the CPU
   specification passes it;
5. the front end and one test per error code.
"""
import numpy as np
import pytest

import ensemble_cases as cases
import ensemble_reference as ens
import posterior_reference as R
import smc_reference as smc
from test_gpu_posterior import BOX1, HI3, LO3, _reference

pytestmark = pytest.mark.gpu

TIE = 1e-9
EPS = 2.0 ** -52
COUNTERS = ("accepted", "outbox", "stuck")
_CACHE = {}


def _model(pkg, nsteps=500, damping=True):
    m = pkg.RateStateModel(number_time_steps=nsteps)
    m.RadiationDamping = damping
    return m


def _bits(x):
    x = np.ascontiguousarray(np.asarray(x.cpu() if hasattr(x, "cpu") else x))
    return x.view(np.int32 if x.dtype.itemsize == 4 else (np.uint8 if x.dtype.itemsize == 1 else np.int64))


def _counters(n):
    return {k: np.zeros(n, dtype=np.int32) for k in COUNTERS}


# ---- 1. the split path against the specification ---------------------------------------------------------------------------------------
def _device_explog_distance(eng, w, lo, hi, B, mask):
    """max over the values w (m, d), inside the box, of |exp_dev(log_dev(w)) - exp_np(log_np(w))| / w in the masked parameters: the
    other half of island 0 holds w, and every mover holds its partner's position, so that u' = fma(z, 0, v) = v and q' = exp(log y)"""
    islands, d = -(-w.shape[0] // B), w.shape[1]
    n = 2 * B * islands
    rows, other = ens.movers(n, B, 0)
    q = np.empty((n, d))
    resting = np.setdiff1d(np.arange(n), rows)
    q[resting] = w[np.arange(resting.size) % w.shape[0]]
    _, _, r = ens.draws(1, rows.astype(np.uint64), 1, B)
    q[rows] = q[other + r]
    qn, inb, _ = eng.ensemble_propose(q, np.zeros(n), lo, hi, 0, log_coords=mask, seed=1, offset=0, iteration=1)
    assert inb[rows].all()
    cols = [p for p in range(d) if (mask >> p) & 1]
    want = np.exp(np.log(q[rows][:, cols]))
    return float((np.abs(qn[rows][:, cols] - want) / want).max())


def _compare_half_step(eng, tag, q, l, cnt, ssq_fn, lo, hi, B, a, mask, shape, seed, offset, it, half, bound, ssq_override=None):
    """One half-step of the GPU's split path IN PLACE in (q, l, cnt), held to the specification applied to the same state →
    dict(margin: the smallest |log alpha - log U_a| of a compared decision, excluded: decisions inside the tie band, eq: the largest
    relative distance of a proposal, spec: the specification's half-step)"""
    n, d = q.shape
    sq, sl, sc = q.copy(), l.copy(), {k: v.copy() for k, v in cnt.items()}
    pr = ens.propose(sq, sl, lo, hi, B, a, mask, seed, offset, it, half, exact=True)
    rows = pr["rows"]
    qn, inb, lj = eng.ensemble_propose(q, l, lo, hi, half, a=a, log_coords=mask, seed=seed, offset=offset, iteration=it)
    rest = np.setdiff1d(np.arange(n), rows)
    np.testing.assert_array_equal(_bits(qn[rest]), _bits(q[rest]), err_msg=f"{tag}: the resting half's q_new rows")
    assert not inb[rest].any() and not lj[rest].any()
    np.testing.assert_array_equal(inb[rows].astype(bool), pr["inbox"], err_msg=f"{tag}: inbox")
    np.testing.assert_array_equal(_bits(qn[rows][pr["stuck"]]), _bits(q[rows][pr["stuck"]]), err_msg=f"{tag}: a stuck walker's q_new is its q")
    assert not lj[rows][pr["stuck"]].any()
    live = ~pr["stuck"]
    if mask == 0:
        np.testing.assert_array_equal(_bits(qn[rows][live]), _bits(pr["q_new"][live]), err_msg=f"{tag}: q' bit for bit")
        eq = 0.0
    else:
        eq = float((np.abs(qn[rows][live] - pr["q_new"][live]) / np.abs(pr["q_new"][live])).max()) if live.any() else 0.0
        assert eq <= bound, f"{tag}: q' within {eq:.3e} (relative), bound {bound:.3e}"
    # J: (d - 1) log z and the masked u' - u, each logarithm within an ulp on either side
    assert np.abs(lj[rows] - pr["J"]).max() <= 1e-12, f"{tag}: J {np.abs(lj[rows] - pr['J']).max():.3e}"
    ssq = np.ones(n)
    ins = inb.astype(bool)
    if ins.any():
        ssq[ins] = ssq_fn(qn[ins])
    sp_ssq = np.ones(rows.size)
    if pr["inbox"].any():
        sp_ssq[pr["inbox"]] = ssq_fn(pr["q_new"][pr["inbox"]])
    if ssq_override is not None:
        for r_, v in ssq_override.items():  # mover index → the value both sides are fed
            ssq[rows[r_]] = v
            sp_ssq[r_] = v
    acc, ln, la = ens.decide(pr, sl, sp_ssq, shape)
    before_q, before_l = q.copy(), l.copy()
    eng.ensemble_accept(q, l, lo, hi, half, qn, inb, lj, ssq, cnt["accepted"], cnt["outbox"], cnt["stuck"], shape, seed=seed, offset=offset, iteration=it)
    np.testing.assert_array_equal(_bits(q[rest]), _bits(before_q[rest]))
    np.testing.assert_array_equal(_bits(l[rest]), _bits(before_l[rest]))
    moved = (_bits(q[rows]) != _bits(before_q[rows])).any(axis=1) | (_bits(l[rows]) != _bits(before_l[rows]))
    grew = {k: cnt[k][rows] - sc[k][rows] for k in COUNTERS}
    with np.errstate(invalid="ignore"):
        margin = np.where(pr["inbox"] & np.isfinite(ln), np.abs(la - pr["log_ua"]), np.inf)
    tie = margin <= TIE
    cmp_ = ~tie
    np.testing.assert_array_equal(grew["accepted"][cmp_] == 1, acc[cmp_], err_msg=f"{tag}: decisions")
    np.testing.assert_array_equal(moved[cmp_] | ~acc[cmp_], np.ones(cmp_.sum(), bool))  # an accepted walker moved (its l at least) ...
    assert not moved[~(grew["accepted"] == 1)].any()                                      # ... and no other did: it keeps its bits
    np.testing.assert_array_equal(grew["outbox"] == 1, ~pr["inbox"] & ~pr["stuck"], err_msg=f"{tag}: outbox")
    np.testing.assert_array_equal(grew["stuck"] == 1, pr["stuck"], err_msg=f"{tag}: stuck")
    assert ((grew["accepted"] + grew["outbox"] + grew["stuck"]) <= 1).all() and all((g >= 0).all() for g in grew.values())
    took = grew["accepted"] == 1
    np.testing.assert_array_equal(_bits(q[rows][took]), _bits(qn[rows][took]), err_msg=f"{tag}: an accepted state is the GPU's own proposal")
    if took.any():
        el = np.abs(l[rows][took] - (-shape * np.log(ssq[rows][took])))
        assert (el <= 4 * EPS * np.abs(l[rows][took]) + 4 * EPS * shape).all(), f"{tag}: l' {el.max():.3e}"
    return dict(margin=float(margin[cmp_].min()) if cmp_.any() else np.inf, excluded=int(tie.sum()), eq=eq, spec=pr, accepted=acc)


def _closed_problem(d):
    c = R.CLOSED[3]
    fn = R.quadratic_ssq(c["S0"], c["q0"][:d], np.asarray(c["K"])[:d, :d])
    lo, hi = np.array([0.2, 1.4, 2.5])[:d], np.array([10.0, 2.6, 3.1])[:d]
    return cases.rows_fn(fn, d), lo, hi, c["shape"]


@pytest.mark.parametrize("d,mask", [(1, 0), (1, 0b001), (2, 0), (2, 0b011), (2, 0b001), (3, 0), (3, 0b011), (3, 0b001)])
def test_split_path_against_the_specification(pkg, d, mask):
    B, islands, n_iter, a, seed, offset = 64, 2, 4, 2.0, 13, 700
    ssq_fn, lo, hi, shape = _closed_problem(d)
    n = 2 * B * islands
    rng = np.random.default_rng(100 + d)
    q = np.ascontiguousarray(rng.uniform(lo, hi, (n, d)))
    l = ens.start_l(q, ssq_fn, shape)
    cnt = _counters(n)
    with pkg.Engine(mem="host", block_threads=B) as eng:
        assert eng.island_size == 2 * B
        bound = 0.0
        if mask:
            # the proposals this run will make (the specification's, from the start state) are the inputs of the measurement
            w = np.concatenate([ens.propose(q, l, lo, hi, B, a, mask, seed, offset, 1, h, exact=False)["q_new"] for h in (0, 1)])
            w = w[smc.inbox(w, lo, hi)]
            dist = _device_explog_distance(eng, w, lo, hi, B, mask)
            bound = 8 * dist
        margin, excluded, eq, accepted = np.inf, 0, 0.0, 0
        for it in range(1, n_iter + 1):
            for half in (0, 1):
                out = _compare_half_step(eng, f"d {d} mask {mask:#05b} it {it} half {half}", q, l, cnt, ssq_fn, lo, hi, B, a, mask, shape, seed, offset,
                                         it, half, bound)
                margin, excluded, eq, accepted = min(margin, out["margin"]), excluded + out["excluded"], max(eq, out["eq"]), accepted + int(out["accepted"].sum())
    print(f"d {d} mask {mask:#05b}: {accepted} accepted of {n * n_iter}, outbox {int(cnt['outbox'].sum())}, smallest margin {margin:.3e}, "
          f"{excluded} decisions inside the tie band, q' within {eq:.3e}" + (f" (exp o log distance {dist:.3e}, bound {bound:.3e})" if mask else " (bit for bit)"))
    assert accepted > 0 and cnt["outbox"].sum() > 0 and cnt["stuck"].sum() == 0 and excluded <= 1


def constructed_rows(B=64, d=3):
    """A two-island state in which, in half-step 0 of iteration 1, movers 0 .. 6 d - 1 of island 0 sit next to a face of the box with
    the whole other half on the far side (so a stretch z > 1 leaves through that face), movers 40 and 41 are stuck (outside the box;
    l = -inf), 42 has l = NaN, and movers 44 .. 47 are fed SSq' = inf, NaN, 0 and -1 → (q, l, lo, hi, shape, ssq_fn, overrides)"""
    ssq_fn, lo, hi, shape = _closed_problem(d)
    n = 4 * B
    rng = np.random.default_rng(3)
    mid, width = 0.5 * (lo + hi), hi - lo
    q = mid + 0.2 * width * rng.uniform(-1.0, 1.0, (n, d))
    for f in range(2 * d):
        p, up = f // 2, f % 2
        for k in range(3):
            q[3 * f + k, p] = (hi[p] - 1e-9 * width[p]) if up else (lo[p] + 1e-9 * width[p])
    l = ens.start_l(q, ssq_fn, shape)
    q[40, 0] = hi[0] + 1.0
    l[41], l[42] = -np.inf, np.nan
    return q, l, lo, hi, shape, ssq_fn, {44: np.inf, 45: np.nan, 46: 0.0, 47: -1.0}


CONSTRUCTED_SEED = 5


def test_split_path_on_constructed_rows(pkg):
    B, d, a = 64, 3, 2.0
    q, l, lo, hi, shape, ssq_fn, over = constructed_rows(B, d)
    cnt = _counters(q.shape[0])
    with pkg.Engine(mem="host", block_threads=B) as eng:
        out = _compare_half_step(eng, "constructed", q, l, cnt, ssq_fn, lo, hi, B, a, 0, shape, CONSTRUCTED_SEED, 0, 1, 0, 0.0, ssq_override=over)
        pr = out["spec"]
        for p in range(d):  # a proposal outside each face
            assert (pr["q_new"][:, p] >= hi[p]).any() and (pr["q_new"][:, p] <= lo[p]).any(), p
        assert pr["stuck"][[40, 41, 42]].all() and pr["stuck"].sum() == 3 and cnt["stuck"][[40, 41, 42]].tolist() == [1, 1, 1]
        assert pr["inbox"][list(over)].all() and not out["accepted"][list(over)].any()
        assert not any(cnt[k][list(over)].any() for k in COUNTERS)  # rejected inside the box: no counter grows
        own = (pr["partner"] % B) == (pr["rows"] % B)  # a mover whose partner is the walker of its own lane
        assert own.any() and (own & pr["inbox"]).any()
        # half-step 1: a stuck walker is drawn as a partner and enters the proposal as it is
        out1 = _compare_half_step(eng, "constructed half 1", q, l, cnt, ssq_fn, lo, hi, B, a, 0, shape, CONSTRUCTED_SEED, 0, 1, 1, 0.0)
        assert np.isin(out1["spec"]["partner"], [40, 41, 42]).any()
    print(f"constructed: outbox {int(cnt['outbox'].sum())}, stuck {int(cnt['stuck'].sum())}, partner = own lane in {int(own.sum())} movers")


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


def _walkers(d, n, seed):
    rng = np.random.default_rng(seed)
    q = np.column_stack([rng.uniform(700.0, 1500.0, n), rng.uniform(0.0095, 0.0125, n), rng.uniform(0.0135, 0.0165, n)])[:, :d]
    q[:8, 0] = np.linspace(1599.0, 1599.9, 8)  # next to the edge: some proposals leave
    return np.ascontiguousarray(q)


FUSED_CASES = {
    "d1": dict(d=1, mask=0, damping=True, groups=1, substeps=1),
    "d3 log": dict(d=3, mask=0b011, damping=True, groups=1, substeps=1),
    "d3 log, two series, undamped": dict(d=3, mask=0b011, damping=False, groups=2, substeps=1),
    "d1, two chunks": dict(d=1, mask=0, damping=True, groups=1, substeps=8),
}


@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_fused_against_split_on_the_real_model(pkg, cpu_engine, name):
    c = FUSED_CASES[name]
    d, mask, G, B, a, seed, offset = c["d"], c["mask"], c["groups"], 64, 2.0, 5, 900
    n = 2 * B * 2
    data = _observations(pkg, cpu_engine, (1000.0, 1200.0)[:G], c["substeps"])
    data = data[0] if G == 1 else data
    lo, hi = np.array([600.0, 0.009, 0.013])[:d], np.array([1600.0, 0.013, 0.017])[:d]
    shape = 0.5 * data.shape[-1]
    q0 = _walkers(d, n, 7)
    names = ("q", "l") + COUNTERS

    with pkg.Engine(mem="host", block_threads=B) as eng:
        eng.set_model(_model(pkg, damping=c["damping"]), c["substeps"])
        l0 = -shape * np.log(np.asarray(eng.fit_normal(q0, data)[0]))
        fused = dict(q=q0.copy(), l=l0.copy(), **_counters(n))
        split = {k: v.copy() for k, v in fused.items()}
        once = {k: v.copy() for k, v in fused.items()}
        rows, far = [], 0.0
        for it in range(1, 5):
            tq, tl = eng.ensemble_run(fused["q"], fused["l"], data, lo, hi, 1, *(fused[k] for k in COUNTERS), a=a, log_coords=mask, shape=shape, seed=seed,
                                      offset=offset, iter0=it, trace=True)
            for half in (0, 1):
                qn, inb, lj = eng.ensemble_propose(split["q"], split["l"], lo, hi, half, a=a, log_coords=mask, seed=seed, offset=offset, iteration=it)
                sn = eng.ensemble_ssq(qn, inb, data, half)
                ins = inb.astype(bool)
                if ins.any():  # any other solve of the same points agrees to rounding (tier 1's bound on SSq), not to the bit
                    other = np.asarray(eng.fit_normal(qn, data)[0])
                    far = max(far, float((np.abs(other[ins] - sn[ins]) / sn[ins]).max()))
                eng.ensemble_accept(split["q"], split["l"], lo, hi, half, qn, inb, lj, sn, *(split[k] for k in COUNTERS), shape, seed=seed, offset=offset,
                                    iteration=it)
            same = {k: bool(np.array_equal(_bits(fused[k]), _bits(split[k]))) for k in names}
            print(f"{name} iteration {it}: accepted so far {int(fused['accepted'].sum())}, outbox {int(fused['outbox'].sum())} of {it * n}; bit-identical {same}")
            assert all(same.values()), same
            assert tq[0].tobytes() == fused["q"].tobytes() and tl[0].tobytes() == fused["l"].tobytes()
            rows.append((tq[0].copy(), tl[0].copy()))
        assert fused["accepted"].sum() > 0 and fused["outbox"].sum() > 0 and fused["stuck"].sum() == 0
        print(f"{name}: rsf_fit_normal's SSq of the same proposals within {far:.3e} (relative) of rsf_ensemble_ssq's")
        assert far <= 1e-9
        assert (fused["accepted"] + fused["outbox"] <= 4).all()
        # four iterations inside one launch: the bits of four launches of one, the trace rows too
        tq, tl = eng.ensemble_run(once["q"], once["l"], data, lo, hi, 4, *(once[k] for k in COUNTERS), a=a, log_coords=mask, shape=shape, seed=seed,
                                  offset=offset, iter0=1, trace=True)
        for k in names:
            np.testing.assert_array_equal(_bits(once[k]), _bits(fused[k]), err_msg=k)
        for it in range(4):
            assert tq[it].tobytes() == rows[it][0].tobytes() and tl[it].tobytes() == rows[it][1].tobytes()
    # device memory: the same bits
    import torch

    with pkg.Engine(mem="device", block_threads=B) as dev:
        dev.set_model(_model(pkg, damping=c["damping"]), c["substeps"])
        st = dict(q=dev._in(q0), l=dev._in(l0), **{k: dev._ints(np.zeros(n)) for k in COUNTERS})
        tq, tl = dev.ensemble_run(st["q"], st["l"], data, lo, hi, 4, *(st[k] for k in COUNTERS), a=a, log_coords=mask, shape=shape, seed=seed, offset=offset,
                                  iter0=1, trace=True)
        torch.cuda.synchronize()
        for k in names:
            np.testing.assert_array_equal(_bits(st[k]), _bits(fused[k]), err_msg=f"device memory: {k}")
        assert np.asarray(tq.cpu())[3].tobytes() == fused["q"].tobytes()


# ---- 3. island identity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [128, 256])
def test_island_identity(pkg, cpu_engine, B):
    data = _observations(pkg, cpu_engine, (1000.0,), 1)[0]
    d, lo, hi, islands = 3, np.array([600.0, 0.009, 0.013]), np.array([1600.0, 0.013, 0.017]), 3
    n = 2 * B * islands
    q0 = _walkers(d, n, 9)
    with pkg.Engine(mem="host", block_threads=B) as eng:
        eng.set_model(_model(pkg), 1)
        assert eng.island_size == 2 * B
        whole = eng.ensemble(q0, data, lo, hi, 3, log_coords=(True, True, False), seed=4, offset=1000, iters_per_launch=2)
        assert whole.island_size == 2 * B and whole.n_islands == islands and whole.trace_q.shape == (3, n, d) and whole.accepted.sum() > 0
        for k in range(islands):
            s = slice(k * 2 * B, (k + 1) * 2 * B)
            alone = eng.ensemble(q0[s], data, lo, hi, 3, log_coords=(True, True, False), seed=4, offset=1000 + k * 2 * B, iters_per_launch=3)
            for f in ("q", "l") + COUNTERS:
                np.testing.assert_array_equal(_bits(getattr(alone, f)), _bits(getattr(whole, f)[s]), err_msg=f"B {B} island {k}: {f}")
            np.testing.assert_array_equal(_bits(alone.trace_q), _bits(whole.trace_q[:, s]))
            np.testing.assert_array_equal(_bits(alone.trace_l), _bits(whole.trace_l[:, s]))
        # the trace's last row is the state; a row differs from the one before exactly where the walker accepted
        np.testing.assert_array_equal(whole.trace_q[-1], whole.q)
        steps = np.concatenate([q0[None], whole.trace_q])
        lsteps = np.concatenate([np.full((1, n), np.nan), whole.trace_l])
        moved = (steps[1:] != steps[:-1]).any(axis=2) | (_bits(lsteps[1:]) != _bits(lsteps[:-1]))
        assert (moved[1:].sum(axis=0) <= whole.accepted).all() and (whole.accepted + whole.outbox + whole.stuck <= 3).all()


# ---- 4. targets -------------------------------------------------------------------------------------------------------------------------------
def _held_to_target(tag, ref, res, eng, island, fails, pooled_fails):
    for row, it in enumerate(res.iterations):
        q = res.trace_q[row]
        std2 = eng.smc_std2(res.trace_l[row], res.shape, res.seed, res.offset, int(it))
        std2 = np.asarray(std2.cpu() if hasattr(std2, "cpu") else std2)
        ens.island_check(f"{tag} iteration {it}", ref, R.quantities(q, std2), island, fails, cases.Z_ISLAND)
        R.check(f"pooled {tag} iteration {it}", ref, q, std2, pooled_fails)


@pytest.mark.parametrize("name,mask", [(n, m) for n, (_, _, masks) in cases.TARGETS.items() for m in masks])
def test_targets_through_the_split_path(gpu_engine, name, mask):
    islands, island, cps = cases.GPU_SSQ_SIZE
    mk, d, _ = cases.TARGETS[name]
    ref, fn, c = mk()
    assert gpu_engine.island_size == island
    q0 = ref.draw(np.random.default_rng(cases.SEED), islands * island)
    res = gpu_engine.ensemble_from_ssq(cases.rows_fn(fn, d), q0, c["lo"], c["hi"], max(cps), c["shape"], log_coords=mask, seed=cases.SEED,
                                       keep=max(cps) - min(cps) + 1, thin=max(cps) - min(cps))
    assert res.iterations.tolist() == list(cps)
    fails, pooled = [], []
    _held_to_target(f"{name} mask {mask:#05b}", ref, res, gpu_engine, island, fails, pooled)
    print(f"{name} mask {mask:#05b}: accept rate {res.accept_rate:.3f}, outside the box {res.outbox_rate:.3f}; pooled check: {pooled or 'passed'}")
    assert res.stuck.sum() == 0 and res.accepted.sum() > 0
    assert not fails, fails
    if cases.POOLED_ASSERTED[name]:
        assert not pooled, pooled


@pytest.mark.parametrize("d", [1, 3])
def test_real_model_targets(pkg, cpu_engine, d):
    lo, hi = (BOX1[0], BOX1[1]) if d == 1 else (LO3, HI3)
    ref, data = _reference(pkg, cpu_engine, d, lo, hi)
    islands, island = 128, 512
    q0 = ref.draw(np.random.default_rng(61 + d), islands * island)
    fails, pooled = [], []
    with pkg.Engine(mem="device") as eng:
        eng.set_model(_model(pkg), 1)
        assert eng.island_size == island
        res = eng.ensemble(q0, data, lo, hi, 20, log_coords=0b011 if d == 3 else None, seed=31 + d, keep=11, thin=10, iters_per_launch=10)
        assert res.iterations.tolist() == [10, 20]
        _held_to_target(f"real d {d}", ref, res, eng, island, fails, pooled)
    print(f"real d {d}: accept rate {res.accept_rate:.3f}, outside the box {res.outbox_rate:.3f}; pooled check (reported): {pooled or 'passed'}")
    assert res.stuck.sum() == 0 and res.accepted.sum() > 0
    assert not fails, fails


# ---- 5. the front end and the contracts ---------------------------------------------------------------------------------------------------------
def test_sample_ensemble_returns_a_posterior_pool(pkg, cpu_engine):
    ref, data = _reference(pkg, cpu_engine, 1, *BOX1)
    mc = pkg.MCMC(_model(pkg), data, 1000.0, ["Uniform", BOX1[0], BOX1[1]], 1000.0)
    pool = mc.sample_ensemble(600, 40, start="smc", seed=6)  # 600 walkers: two islands of 512; SMC's particles are a draw of pi
    assert isinstance(pool, pkg.PosteriorPool) and pool.samples.shape == (20, 1024, 1) and pool.std2.shape == (20, 1024) and pool.nburn == 20
    assert pool.stats["n_walkers"] == 1024 and pool.stats["island_size"] == 512 and pool.stats["n_islands"] == 2 and pool.stats["logmask"] == 0
    diag = pool.diagnostics()[0]
    mg = ref.marg["Dc"]
    z = (pool.samples.mean() - mg.mean) / (mg.sd / np.sqrt(diag["ess"]))
    print(f"sample_ensemble: accept rate {pool.accept_rate:.3f}, Dc mean {pool.samples.mean():.2f} against {mg.mean:.2f} (sd {mg.sd:.2f}), ESS "
          f"{diag['ess']:.0f} of {20 * 1024}, diagnostics { {k: v for k, v in diag.items() if 'rhat' in k} }, z {z:+.2f}")
    assert np.isfinite(pool.std2).all() and (pool.std2 > 0).all() and pool.stats["stuck"] == 0 and 0 < pool.accept_rate <= 1
    assert pool.stats["smc_stages"] > 0 and abs(z) < R.Z_MAX
    pool = mc.sample_ensemble(100, 8, start="fit", seed=6, thin=2)  # a ball around the least-squares estimate: the bookkeeping only
    assert pool.samples.shape == (2, 512, 1) and pool.nburn == 4 and "fit" in pool.stats and pool.stats["stuck"] == 0
    pool = mc.sample_ensemble(512, 6, start=np.full((512, 1), 1000.0) + np.linspace(-50.0, 50.0, 512)[:, None], nburn=2, thin=2)
    assert pool.samples.shape == (2, 512, 1) and "fit" not in pool.stats


def _code(pkg, call):
    with pytest.raises(pkg.RsfError) as ei:
        call()
    return ei.value.code


def _state(n, d=1, l=0.0):
    q = np.ascontiguousarray(np.linspace(900.0, 1100.0, n * d).reshape(n, d))
    return dict(q=q, l=np.full(n, float(l)), **_counters(n))


def _run(eng, st, **kw):
    a = dict(data=np.zeros(500), lo=BOX1[0], hi=BOX1[1], n_iter=1, a=2.0, log_coords=None, shape=250.0, seed=0, offset=0, iter0=1)
    a.update(kw)
    return eng.ensemble_run(st["q"], st["l"], a.pop("data"), a.pop("lo"), a.pop("hi"), a.pop("n_iter"), *(st[k] for k in COUNTERS), **a)


def test_error_state_without_a_model(pkg):
    with pkg.Engine(mem="host", block_threads=64) as eng:
        with pytest.raises(pkg.RsfError) as ei:
            _run(eng, _state(128))
        assert ei.value.code == -3
        assert _code(pkg, lambda: eng.ensemble_ssq(np.ones((128, 1)), np.ones(128, np.uint8), np.zeros(500), 0)) == -3


def test_error_invalid_arguments(pkg):
    P = lambda x: x.ctypes.data
    dp = lambda v: np.array([v], dtype=np.float64).ctypes.data_as(pkg._abi._DP)
    with pkg.Engine(mem="host", block_threads=64) as eng:
        eng.set_model(_model(pkg), 1)
        st = _state(128)
        _run(eng, st)
        for kw in (dict(n_iter=0), dict(n_iter=65), dict(iter0=0), dict(iter0=2 ** 32), dict(offset=-1), dict(a=1.0), dict(a=0.5), dict(a=np.inf),
                   dict(a=np.nan), dict(shape=0.0), dict(shape=np.nan), dict(lo=5.0, hi=5.0), dict(hi=np.inf), dict(lo=-1.0, log_coords=1),
                   dict(data=np.zeros((2, 500)))):  # one island over two series
            assert _code(pkg, lambda: _run(eng, st, **kw)) == -1, kw
        assert _code(pkg, lambda: _run(eng, _state(64))) == -1    # half an island
        assert _code(pkg, lambda: _run(eng, _state(192))) == -1   # one and a half
        assert _code(pkg, lambda: _run(eng, _state(128, 2))) == -1  # the solve has d = 1 or 3
        lib, ctx = eng.lib, eng._ctx
        ok = [ctx, 128, 1, P(st["q"]), P(st["l"]), P(np.zeros(500)), 1, dp(0.0), dp(1e4), 2.0, 0, 250.0, 0, 0, 1, 1, P(st["accepted"]), P(st["outbox"]),
              P(st["stuck"]), None, None]
        assert lib.rsf_ensemble_run(*ok) == 0
        for i, v in ((1, 0), (2, 2), (2, 4), (3, None), (4, None), (5, None), (6, 0), (7, None), (10, 2), (16, None), (18, None), (19, P(st["q"]))):
            bad = list(ok)
            bad[i] = v
            assert lib.rsf_ensemble_run(*bad) == -1, i
        assert lib.rsf_ensemble_run(None, *ok[1:]) == -1
        qn, inb, _ = eng.ensemble_propose(st["q"], st["l"], *BOX1, 0)
        assert eng.ensemble_ssq(qn, inb, np.zeros(500), 0).shape == (128,)
        for call in (lambda: eng.ensemble_ssq(qn, inb, np.zeros(500), 2), lambda: eng.ensemble_ssq(qn, inb, np.zeros((2, 500)), 0),
                     lambda: eng.ensemble_ssq(qn[:64], inb[:64], np.zeros(500), 0), lambda: eng.ensemble_ssq(np.ones((128, 2)), inb, np.zeros(500), 0)):
            assert _code(pkg, call) == -1
        assert lib.rsf_ensemble_ssq(ctx, 128, 1, None, P(inb), P(np.zeros(500)), 1, 0, P(np.ones(128))) == -1
        # the Python layer refuses before any library call
        with pytest.raises(ValueError, match="whole islands"):
            eng.ensemble(np.full(100, 1000.0), np.zeros(500), *BOX1, 2)
        with pytest.raises(ValueError, match="stuck start"):
            eng.ensemble(np.full(128, 2.0e4), np.zeros(500), *BOX1, 2)
    # the split calls: d = 1..3, no model needed
    with pkg.Engine(mem="host", block_threads=64) as bare:
        st = _state(128, 2)
        lo, hi = [0.0, 0.0], [1e4, 1e4]
        qn, inb, lj = bare.ensemble_propose(st["q"], st["l"], lo, hi, 0)
        assert inb.shape == (128,) and lj.shape == (128,)
        bare.ensemble_accept(st["q"], st["l"], lo, hi, 0, qn, inb, lj, np.ones(128), *(st[k] for k in COUNTERS), 250.0)
        for half in (-1, 2):
            assert _code(pkg, lambda: bare.ensemble_propose(st["q"], st["l"], lo, hi, half)) == -1
            assert _code(pkg, lambda: bare.ensemble_accept(st["q"], st["l"], lo, hi, half, qn, inb, lj, np.ones(128), *(st[k] for k in COUNTERS), 250.0)) == -1
        for kw in (dict(a=1.0), dict(a=np.nan), dict(offset=-1), dict(iteration=0), dict(iteration=2 ** 32)):
            assert _code(pkg, lambda: bare.ensemble_propose(st["q"], st["l"], lo, hi, 0, **kw)) == -1, kw
        for kw in (dict(offset=-1), dict(iteration=0), dict(iteration=2 ** 32)):
            assert _code(pkg, lambda: bare.ensemble_accept(st["q"], st["l"], lo, hi, 0, qn, inb, lj, np.ones(128), *(st[k] for k in COUNTERS), 250.0, **kw)) == -1, kw
        with pytest.raises(ValueError, match="beyond d"):
            bare.ensemble_propose(st["q"], st["l"], lo, hi, 0, log_coords=0b100)
        assert bare.lib.rsf_ensemble_propose(bare._ctx, 128, 2, P(st["q"]), P(st["l"]), np.array(lo).ctypes.data_as(pkg._abi._DP),
                                             np.array(hi).ctypes.data_as(pkg._abi._DP), 2.0, 0b100, 0, 0, 1, 0, P(qn), P(inb), P(lj)) == -1  # a mask bit at d
        assert bare.lib.rsf_ensemble_propose(bare._ctx, 128, 2, P(st["q"]), P(st["l"]), np.array([-1.0, 0.0]).ctypes.data_as(pkg._abi._DP),
                                             np.array(hi).ctypes.data_as(pkg._abi._DP), 2.0, 0b001, 0, 0, 1, 0, P(qn), P(inb), P(lj)) == -1  # lo < 0 under a bit
        assert _code(pkg, lambda: bare.ensemble_accept(st["q"], st["l"], lo, hi, 0, qn, inb, lj, np.ones(128), *(st[k] for k in COUNTERS), 0.0)) == -1
        z4 = np.ones((128, 4))
        assert bare.lib.rsf_ensemble_propose(bare._ctx, 128, 4, P(z4), P(st["l"]), np.zeros(4).ctypes.data_as(pkg._abi._DP),
                                             np.full(4, 2.0).ctypes.data_as(pkg._abi._DP), 2.0, 0, 0, 0, 1, 0, P(z4.copy()), P(inb), P(lj)) == -1
        assert bare.lib.rsf_ensemble_propose(bare._ctx, 128, 2, None, None, None, None, 2.0, 0, 0, 0, 1, 0, None, None, None) == -1
        assert b"NULL" in bare.lib.rsf_last_error()


def test_error_unsupported_integrator_and_the_float32_model(pkg):
    with pkg.Engine(mem="host", block_threads=64) as eng:
        m = _model(pkg)
        m.integrator = "dop853"
        eng.set_model(m, 1)
        st = _state(128)
        assert _code(pkg, lambda: _run(eng, st)) == -5
        assert eng.lib.rsf_ensemble_ssq(eng._ctx, 128, 1, st["q"].ctypes.data, np.ones(128, np.uint8).ctypes.data, np.zeros(500).ctypes.data, 1, 0, np.ones(128).ctypes.data) == -5
        # a float32 model gets the float64 solve: the bits of the float64 model
        data = np.cos(np.linspace(0.0, 3.0, 500))
        m = _model(pkg)
        m.precision = "float32"
        eng.set_model(m, 1)
        a = _state(128, l=-1e9)  # far below any l': the first proposals inside the box are accepted, so the solve's bits reach l
        _run(eng, a, data=data, n_iter=2)
        eng.set_model(_model(pkg), 1)
        b = _state(128, l=-1e9)
        _run(eng, b, data=data, n_iter=2)
        for k in ("q", "l") + COUNTERS:
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)
        assert b["accepted"].sum() > 0 and (b["l"] > -1e9).any()
