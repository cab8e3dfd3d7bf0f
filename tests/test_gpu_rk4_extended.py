"""
GPU tests: the float64 RK4 kernels — every tier (TIGHT, NARROW, WIDE, FULL) and the events between them (handover, cold
redo, resync, FULL retry, tier exit) — against the extended-precision RK4 reference (tests/rk4_extended.py), at the
accuracy a plain float64 RK4 reaches.

The design's claim is that each incremental tier is exact to rounding inside its guard (csrc/rsf_device.h, the truncation
table above struct Guard).  The restatement parity tests compare at 1e-9 with a float64 restatement whose own rounding is
the GPU's size; a series cut one term short or a guard set too wide costs 1e-14 .. 1e-11 per solve and passes there.  Here
the yardstick is the CPU restatement's own distance from the exact scheme, measured in the same test on the same lanes:
the kernel may be at most a small fixed factor further away, and under an absolute cap.

Lane sets (rk4_extended.place_lanes): whole waves of 64 lanes placed by the kernel's own a-priori tier bound.  Models:
rk4_extended.CASES.  Extended solves are cached per model for the module: the CPU side bounds the run time.
"""
import numpy as np
import pytest

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
