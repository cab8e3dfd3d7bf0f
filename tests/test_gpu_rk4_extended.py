"""
GPU tests: the float64 RK4 kernels — every tier (TIGHT, NARROW, WIDE, FULL) and the events between them (handover, cold
redo, resync, FULL retry, tier exit) — against the extended-precision RK4 reference (tests/rk4_extended.py), at the
accuracy a plain float64 RK4 reaches.

The design's claim is that each incremental tier is exact to rounding inside its guard (csrc/rsf_device.h, the truncation
table above struct Guard).  The restatement parity tests compare at 1e-9 with a float64 restatement whose own rounding is
the GPU's size; a series cut one term short or a guard set too wide costs 1e-14 .. 1e-11 per solve and passes there.  Here
the yardstick is the CPU restatement's own distance from the exact scheme, measured in the same test on the same lanes:
the kernel may be at most a small fixed factor further away, and under an absolute cap.

The init kernel (ssq0, std2_0 and the proposal covariance of compute_initial_covariance; float64 and float32 modes, with
observation groups) is held the same way against the extended init of tests/init_extended.py.

Lane sets (rk4_extended.place_lanes): whole waves of 64 lanes placed by the kernel's own a-priori tier bound.  Models:
rk4_extended.CASES.  Extended solves are cached per model for the module: the CPU side bounds the run time.
"""
import numpy as np
import pytest

import init_extended as I
import rk4_extended as X

pytestmark = pytest.mark.gpu

# float64 forward kernel and sampler SSq against the extended reference.  Per set: max and median of the GPU's per-lane
# error within FACTOR x the CPU restatement's on the same lanes (FACTOR x FLOOR where the restatement is at rounding level
# itself), and the max under the absolute caps.  Measured on MI355X over every case, set and (a, b) variant here: GPU/restatement
# ratio at most 1.6 (trajectory) and 3.9 (SSq, against the floor); GPU error at most 5.9e-13 (trajectory, n2000_S2_mu-4e-4
# tight) and 8.1e-14 (SSq, n500_S3 wide) — the mixed-tier path is as accurate as a plain float64 RK4.  Margins 2.5x / 2x on
# the factors, 3.4x / 6x on the caps (today's parity tolerance: 1e-9).
FACTOR_TRAJ, FACTOR_SSQ = 4.0, 8.0
TRAJ_FLOOR, SSQ_FLOOR = 2e-14, 1e-14
TRAJ_CAP, SSQ_CAP = 2e-12, 5e-13
# float32 solve against the extended reference, per form.  Measured max (trajectory / SSq): incremental form (tight, tight_edge,
# narrow sets) 2.3e-5 / 2.3e-5 (nondefault narrow; 3.4e-6 with the default constants), full evaluations (full set) 3.1e-5 /
# 1.6e-5, the wide set (chains switching form mid-solve) 6.8e-5 / 3.1e-5.  Margins 2.9x .. 4.3x.
F32_CAPS = {"tight": (1e-4, 1e-4), "tight_edge": (1e-4, 1e-4), "narrow": (1e-4, 1e-4), "full": (1e-4, 1e-4), "wide": (2e-4, 1e-4)}

_PROBLEMS, _ORACLE = {}, {}


def _problem(oracle_mod, name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = X.Problem(oracle_mod.ModelSpec, name)
    return _PROBLEMS[name]


def _oracle_errors(cpu_engine, p, variant):
    """the CPU restatement's per-lane errors on problem p (cached with it)"""
    key = (p.name, variant)
    if key not in _ORACLE:
        assert cpu_engine.set_model(p.m, p.m.substeps) == p.data.size
        ssq, acc = cpu_engine.forward(p.dc, data=p.data, want_ssq=True, want_acc=True, **p.kw(variant))
        _ORACLE[key] = X.rel_errors(acc, ssq, *p.ext[variant])
    return _ORACLE[key]


def _check(tag, g, o, factor, floor, cap, fails):
    """g, o: per-lane errors of GPU and restatement on one set"""
    gm, gd, om, od = g.max(), np.median(g), o.max(), np.median(o)
    print(f"{tag}: gpu max {gm:.2e} med {gd:.2e} | oracle max {om:.2e} med {od:.2e} | ratio max {gm / max(om, floor):.1f} "
          f"med {gd / max(od, floor):.1f}")
    if not (gm <= factor * max(om, floor) and gd <= factor * max(od, floor) and gm < cap):
        fails.append(tag)


@pytest.mark.parametrize("name", list(X.CASES))
def test_forward_tiers_within_float64_rounding(gpu_engine, cpu_engine, oracle_mod, name):
    """The forward kernel (trajectory and SSq, one launch) on every lane set, with and without per-lane (a, b)."""
    p = _problem(oracle_mod, name)
    fails = []
    for variant in ("plain", "ab"):
        ot, os_ = _oracle_errors(cpu_engine, p, variant)
        assert gpu_engine.set_model(p.m, p.m.substeps) == p.data.size
        ssq, acc = gpu_engine.forward(p.dc, data=p.data, want_ssq=True, want_acc=True, **p.kw(variant))
        gt, gs = X.rel_errors(acc, ssq, *p.ext[variant])
        for s in p.sets:
            sl = p.lanes(s)
            _check(f"{name} {variant} {s} traj", gt[sl], ot[sl], FACTOR_TRAJ, TRAJ_FLOOR, TRAJ_CAP, fails)
            _check(f"{name} {variant} {s} ssq", gs[sl], os_[sl], FACTOR_SSQ, SSQ_FLOOR, SSQ_CAP, fails)
    assert not fails, fails


SAMPLER_CASES = ["n500_S1", "n500_S3_nodamp", "n2000_S1", "n500_S1_k1zero", "nondefault", "n500_S1_mu+5e-4", "n4000_S1_mu+5e-4"]


def _sampler_ssq(engine, p, s, d, replay):
    """One sampler iteration with forced acceptance on set s: a proposal covariance (1e-7 q)^2 and sigma^2 = 1e300 put the
    Metropolis ratio at exp(-0) (early rejection can never fire).  d = 1: q = Dc with the model's (a, b); d = 3: q = (Dc, a, b)
    with the "ab" variant's per-lane b.  replay: mcmc_replay with z = 0 (the proposal is the start point itself) and u = 1e-300
    — the REPLAY instantiation — else mcmc_run(1), the production instantiation with Philox variates.
    -> (q of the proposal (C, d), the sampler's own SSq at it, accept flags, counter deltas of the iteration)"""
    sl = p.lanes(s)
    C = X.WAVE
    q0 = p.dc[sl].reshape(C, 1) if d == 1 else np.stack([p.dc[sl], p.a[sl], p.b[sl]], axis=1)
    lo, hi = [0.0] * d, [100.0 * p.dc.max()] + [1.0] * (d - 1)
    engine.mcmc_init(q0, p.data, lo, hi, seed=17, prior_len=3)
    V = np.zeros((C, d, d))
    for k in range(d):
        V[:, k, k] = (1e-7 * q0[:, k]) ** 2
    engine.set_state(q=q0, V=V, std2=np.full(C, 1e300))
    c0 = engine.counters()
    if replay:
        tq, _, ta = engine.mcmc_replay(np.zeros((1, C, d)), np.full((1, C), 1e-300), np.full((1, C), 250.0))
    else:
        tq, _, ta = engine.mcmc_run(1)
    c1 = engine.counters()
    q, ssq = engine.get_state()[:2]
    return np.array(tq[0]), np.array(ssq), np.array(ta[0]), {k: c1[k] - c0[k] for k in c1 if k.startswith("steps")}


def _tier_evidence(p, s, cnt):
    """counters: the set ran the tier it was placed in.  A TIGHT wave at n = 500 runs TIGHT only — but for the chunk's odd
    last step, which takes the WIDE series whatever the tier (rsf_device.h integrate_tiers); at finer steps one early trip of
    it may trip its guard (the a-priori bound covers the mu increment, not rho) and run NARROW until it is calm again.  A
    model with mu_t_zero != mu_ref (the offset cases, and `nondefault`: 0.58 against 0.55) trips from the first trip: redone
    (but for its stiff set, which runs FULL from the start)."""
    if p.m.mu_t_zero != p.m.mu_ref and s != "full":
        return cnt["steps_redone"] > 0
    if s == "tight" and p.m.num_tsteps * p.m.substeps <= 500:
        return cnt["steps_narrow"] == cnt["steps_full"] == cnt["steps_redone"] == 0 and cnt["steps_wide"] <= 1 and cnt["steps_tight"] > 0
    return {"tight": cnt["steps_full"] == 0 and cnt["steps_tight"] > 0, "tight_edge": cnt["steps_tight"] > 0,
            "narrow": cnt["steps_narrow"] > 0, "wide": cnt["steps_wide"] > 0, "full": cnt["steps_full"] > 0}[s]


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("name", SAMPLER_CASES)
def test_sampler_ssq_within_float64_rounding(gpu_engine, cpu_engine, oracle_mod, name, d):
    """The sampler kernels' own solve — d = 1 with its 16-step TIGHT trips, d = 3 (Dc, a, b) — through mcmc_run (Philox) and
    mcmc_replay: get_state()'s SSq at the accepted proposal against the extended reference there, to the forward test's
    tolerance, and the counters show each set ran its tier."""
    p = _problem(oracle_mod, name)
    variant = "plain" if d == 1 else "ab"
    gpu_engine.set_model(p.m, p.m.substeps)
    _, os_ = _oracle_errors(cpu_engine, p, variant)
    fails, runs = [], {}
    for s in p.sets:
        for replay in (False, True):
            q, ssq, acc, cnt = _sampler_ssq(gpu_engine, p, s, d, replay)
            assert acc.all(), f"{name} {s} d={d} replay={replay}: {int((~acc.astype(bool)).sum())} chains did not accept"
            print(f"{name} d={d} {s} replay={replay} counters {cnt}")
            assert _tier_evidence(p, s, cnt), (name, s, d, replay, cnt)
            runs[(s, replay)] = (q, ssq)
    # the extended SSq at the run's proposals (one solve over every set); the replay proposed the start point itself
    qr = np.concatenate([runs[(s, False)][0] for s in p.sets])
    a_q = qr[:, 1] if d == 3 else None
    b_q = qr[:, 2] if d == 3 else None
    _, ssq_run_ext = X.forward_ext(p.m, qr[:, 0], a_q, b_q, data=p.data)
    for i, s in enumerate(p.sets):
        sl = p.lanes(s)
        ext = ssq_run_ext[X.WAVE * i:X.WAVE * (i + 1)]
        for replay, ref in ((False, ext), (True, p.ext[variant][1][sl])):
            g = (np.abs(X._w(runs[(s, replay)][1]) - ref) / ref).astype(np.float64)
            _check(f"{name} d={d} {s} {'replay' if replay else 'run'} ssq", g, os_[sl], FACTOR_SSQ, SSQ_FLOOR, SSQ_CAP, fails)
    assert not fails, fails


F32_CASES = ["n500_S1", "n500_S3_nodamp", "n2000_S1", "n4000_S1", "nondefault"]


@pytest.mark.parametrize("name", F32_CASES)
def test_float32_forward_and_sampler_against_the_reference(gpu_engine, oracle_mod, name):
    """The float32 solve's formulation, per form, against the extended reference (independent of its bit-exact restatement):
    TIGHT/NARROW lanes stay in the incremental form, FULL lanes take full evaluations (their increments are past the
    incremental form's |dlt| < 2^-7)."""
    p = _problem(oracle_mod, name)
    m32 = X.make_model(oracle_mod.ModelSpec, name)
    m32.precision = "float32"
    fails = []
    for variant in ("plain", "ab"):
        gpu_engine.set_model(m32, m32.substeps)
        ssq, acc = gpu_engine.forward(p.dc, data=p.data, want_ssq=True, want_acc=True, **p.kw(variant))
        gt, gs = X.rel_errors(acc, ssq, *p.ext[variant])
        for s in p.sets:
            sl = p.lanes(s)
            print(f"f32 {name} {variant} {s}: traj max {gt[sl].max():.2e} med {np.median(gt[sl]):.2e} | "
                  f"ssq max {gs[sl].max():.2e} med {np.median(gs[sl]):.2e}")
            if not (gt[sl].max() < F32_CAPS[s][0] and gs[sl].max() < F32_CAPS[s][1]):
                fails.append(f"forward {variant} {s}")
    for s in p.sets:
        q, ssq, acc, cnt = _sampler_ssq(gpu_engine, p, s, 1, True)
        assert acc.all()
        sl = p.lanes(s)
        g = (np.abs(X._w(ssq) - p.ext["plain"][1][sl]) / p.ext["plain"][1][sl]).astype(np.float64)
        print(f"f32 {name} sampler {s}: ssq max {g.max():.2e} med {np.median(g):.2e} counters {cnt}")
        if not g.max() < F32_CAPS[s][1]:
            fails.append(f"sampler {s}")
        if m32.substeps == 1:  # the form each set ran (the float32 sampler counts incremental trips as steps_tight, full ones as steps_full)
            form_ok = cnt["steps_full"] == 0 if s in ("tight", "tight_edge") else (cnt["steps_full"] > 0 if s == "full" else True)
            if not (form_ok and cnt["steps_tight"] > 0):
                fails.append(f"sampler {s} form {cnt}")
    assert not fails, fails


# The init kernel (init_kernel: ssq0, std2_0 and the proposal covariance V of compute_initial_covariance) against the extended
# reference of the same init (tests/init_extended.py).  ssq0 and std2_0 are held to the forward test's SSq rules: measured on
# MI355X over every case, set, d, mode and group, GPU error at most 6.3e-14 (nondefault wide, d = 3), ratio at most 3.9
# (against the floor; nondefault full).  V is a forward difference with relative step fd: the trajectories' ~1e-13 rounding,
# divided by fd times the relative sensitivity, is the restatement's own V error — at most 4.2e-7 for d = 1 (fd = 1e-6,
# relative error) and 8.7e-8 for d = 3 (fd = 1e-4, every entry over sqrt(V_pp V_rr)).  Per set: max and median of the GPU's
# per-chain V error within FACTOR_V x the restatement's on the same chains (x V_FLOOR where the restatement is below it),
# and the max under V_CAP (the parity tests: 2e-6 / 1e-4).  V_FLOOR: the restatement's own median on the ordinary (tight)
# sets, d = 1 4e-8 .. 8e-8 — the level a plain float64 RK4 reaches; below it the two float64 solves differ by how their
# rounding correlates between the base and the perturbed trajectory (nondefault's full and wide sets: GPU 9.8e-8 and 1.3e-7
# against the restatement's 2.1e-8 and 2.9e-8, the forward kernel's trajectories giving the same V — the FULL/WIDE step of
# the shared solver, at 2e-14 trajectory error).  Measured: ratio at most 2.7 (d = 1, nondefault wide) and 1.1 (d = 3),
# GPU max 3.7e-7 (d = 1) and 4.0e-8 (d = 3), n4000_S1_mu+5e-4 tight, both below the restatement's on the same chains.
# Margins 2.2x / 5.5x on the factor, 2.7x / 5x on the caps.
FACTOR_V = 6.0
V_FLOOR = {1: 5e-8, 3: 2e-9}
V_CAP = {1: 1e-6, 3: 2e-7}
INIT_FD = {1: 1e-6, 3: 1e-4}
_INIT_REF, _INIT_ORACLE = {}, {}


def _init_inputs(p, d, idx=None):
    """start points of the init tests: d = 1 the plain lanes (q = Dc), d = 3 the ab lanes (q = (Dc, a, b)); the prior box
    lo = (0, 0.005, 0.005), hi = (100 max Dc, 0.02, 0.03).  idx: the lanes (default all), in order"""
    idx = np.arange(p.dc.size) if idx is None else idx
    q0 = p.dc[idx].reshape(-1, 1) if d == 1 else np.stack([p.dc[idx], p.a[idx], p.b[idx]], axis=1)
    return q0, [0.0, 0.005, 0.005][:d], [100.0 * p.dc.max(), 0.02, 0.03][:d]


def _init_ref(p, d, data=None, idx=None, key=None):
    """the extended init at _init_inputs(p, d, idx) (cached under key)"""
    if key is None or key not in _INIT_REF:
        q0, lo, hi = _init_inputs(p, d, idx)
        acc0 = p.ext["plain" if d == 1 else "ab"][0]
        acc0 = acc0 if idx is None else acc0[:, idx]
        ref = I.initial_state_ext(X.forward_ext, p.m, q0, p.data if data is None else data, INIT_FD[d], 3, lo, hi, acc0=acc0)
        if key is None:
            return ref
        _INIT_REF[key] = ref
    return _INIT_REF[key]


def _init_errors(engine, m, p, d, ref, data=None, idx=None):
    """mcmc_init on engine (model m) at _init_inputs(p, d, idx): per-chain errors (ssq0, std2_0, V) against ref"""
    q0, lo, hi = _init_inputs(p, d, idx)
    engine.set_model(m, m.substeps)
    engine.mcmc_init(q0, p.data if data is None else data, lo, hi, seed=17, prior_len=3, fd_rel_step=INIT_FD[d])
    _, ssq, std2, V = engine.get_state()
    return I.rel(ssq, ref[0]), I.rel(std2, ref[1]), I.v_errors(V, ref[2])


def _init_oracle(cpu_engine, p, d):
    key = (p.name, d)
    if key not in _INIT_ORACLE:
        _INIT_ORACLE[key] = _init_errors(cpu_engine, p.m, p, d, _init_ref(p, d, key=key))
    return _INIT_ORACLE[key]


def _check_init(tag, d, g, o, sl, fails, f32_ssq_cap=None):
    """g, o: (ssq0, std2_0, V) per-chain errors of GPU and restatement; sl: the chains of one set.  f32_ssq_cap: the
    float32 mode's ssq0 (ssq32_kernel), held to that cap alone"""
    if f32_ssq_cap is None:
        _check(f"{tag} ssq0", g[0][sl], o[0][sl], FACTOR_SSQ, SSQ_FLOOR, SSQ_CAP, fails)
    else:
        print(f"{tag} ssq0 (float32): gpu max {g[0][sl].max():.2e} med {np.median(g[0][sl]):.2e}")
        if not g[0][sl].max() < f32_ssq_cap:
            fails.append(f"{tag} ssq0 float32")
    _check(f"{tag} std2_0", g[1][sl], o[1][sl], FACTOR_SSQ, SSQ_FLOOR, SSQ_CAP, fails)
    _check(f"{tag} V", g[2][sl], o[2][sl], FACTOR_V, V_FLOOR[d], V_CAP[d], fails)


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("name", list(X.CASES))
def test_init_within_float64_rounding(gpu_engine, cpu_engine, oracle_mod, name, d):
    """init_kernel (float64 mode) — eight-step trips whose tier only moves up, the per-lane cold redo, the chunk tail in
    single WIDE steps, the resync, the cv * dsum samples and the lane group's DPP exchange — on every lane set, in one
    mcmc_init over all of them: a set of 64 chains is 2 whole waves at d = 1, 4 at d = 3, and the a-priori tier placement
    survives the perturbations.  ssq0, std2_0 and V against the extended init."""
    p = _problem(oracle_mod, name)
    o = _init_oracle(cpu_engine, p, d)
    g = _init_errors(gpu_engine, p.m, p, d, _init_ref(p, d, key=(p.name, d)))
    fails = []
    for s in p.sets:
        _check_init(f"{name} d={d} {s}", d, g, o, p.lanes(s), fails)
    assert not fails, fails


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("name", F32_CASES)
def test_float32_init_against_the_reference(gpu_engine, cpu_engine, oracle_mod, name, d):
    """The float32 mode's init: std2_0 and V come from the float64 init kernel (rsf_oracle.c rsf_mcmc_init keeps them
    float64 in that mode) and are held to the float64 rules; ssq0 is ssq32_kernel's float32 solve (the staged-chunk path,
    whatever the forward kernel does), held to F32_CAPS."""
    p = _problem(oracle_mod, name)
    m32 = X.make_model(oracle_mod.ModelSpec, name)
    m32.precision = "float32"
    o = _init_oracle(cpu_engine, p, d)
    g = _init_errors(gpu_engine, m32, p, d, _init_ref(p, d, key=(p.name, d)))
    fails = []
    for s in p.sets:
        _check_init(f"f32 {name} d={d} {s}", d, g, o, p.lanes(s), fails, f32_ssq_cap=F32_CAPS[s][1])
    assert not fails, fails


GROUP_SETS = ("tight", "narrow", "wide", "full")


@pytest.mark.parametrize("precision", ["float64", "float32"])
@pytest.mark.parametrize("d", [1, 3])
def test_init_with_observation_groups(gpu_engine, cpu_engine, oracle_mod, d, precision):
    """Two observation groups of 512 chains (a multiple of both modes' workgroup chains; the init kernel's workgroup holds
    blockDim / (d + 1) chains, select_group's own arithmetic): each group tiles the tight, narrow, wide and full sets twice.
    Group 1 observes a second series — the extended solve at the first narrow lane's Dc plus noise.  Each group is judged
    against the extended init on its own series."""
    p = _problem(oracle_mod, "n500_S1")
    sets = np.concatenate([np.arange(p.dc.size)[p.lanes(s)] for s in GROUP_SETS])
    per = 2 * sets.size
    idx = np.tile(sets, 4)  # 2 copies per group, 2 groups
    acc1, _ = X.forward_ext(p.m, p.dc[p.lanes("narrow")][:1])
    acc1 = acc1[:, 0].astype(np.float64)
    data = np.stack([p.data, acc1 + np.abs(acc1) * np.random.default_rng(5).standard_normal(acc1.size)])
    key = ("groups", d)
    ref = _init_ref(p, d, data=data, idx=idx, key=key)
    if key not in _INIT_ORACLE:
        _INIT_ORACLE[key] = _init_errors(cpu_engine, p.m, p, d, ref, data=data, idx=idx)
    o = _INIT_ORACLE[key]
    m = X.make_model(oracle_mod.ModelSpec, "n500_S1")
    m.precision = precision
    g = _init_errors(gpu_engine, m, p, d, ref, data=data, idx=idx)
    fails = []
    for grp in range(2):
        for i, s in enumerate(GROUP_SETS):
            sl = np.concatenate([grp * per + c * sets.size + np.arange(X.WAVE * i, X.WAVE * (i + 1)) for c in range(2)])
            _check_init(f"groups {precision} d={d} group {grp} {s}", d, g, o, sl, fails,
                        f32_ssq_cap=F32_CAPS[s][1] if precision == "float32" else None)
    assert not fails, fails
