"""
GPU tests: the DOP853 kernels (RSF_FLAG_DOP853, csrc/rsf_device_dop853.h) — the steady-state fast path with its incremental
stages, the guard's redo, the general loop, a failed call — against the extended-precision DOP853 reference
(tests/dop853_extended.py), at the accuracy a plain float64 DOP853 reaches.

The parity tests compare with the float64 C restatement at 1e-9; a series cut one term short, a guard set too wide or a
missing resync costs 1e-14 .. 1e-11 and passes there.  Here the yardstick is the C restatement's own distance from the exact
map, measured in the same test on the same lanes: the kernel may be at most a small fixed factor further away, and under an
absolute cap.  Decision-adjacent lanes (the reference's record: a decision within 1e-5 of its threshold, which the fast
path's ~1e-7 err may take otherwise) are held to the parity tolerance only, and counted.
"""
import numpy as np
import pytest

import dop853_extended as X
import init_extended as I

pytestmark = pytest.mark.gpu

# Per set: max and median of the GPU's per-lane error within FACTOR x the restatement's on the same lanes (x FLOOR where the
# restatement is at rounding level itself), and the max under the caps.  Measured on MI355X over every case, set and variant:
# GPU/restatement ratio at most 1.2 (max and median, trajectory and SSq, forward, init and sampler); the largest errors are
# the restatement's own (2.9e-11 trajectory on the fast sets at the largest Dc, n500_mu+5e-4).
FACTOR_TRAJ, FACTOR_SSQ = 4.0, 8.0
TRAJ_FLOOR, SSQ_FLOOR = 1e-13, 1e-13
TRAJ_CAP, SSQ_CAP = 1e-10, 2e-11
# Stiff lanes (the stiff set, the mixed wave's two) amplify rounding through their step sizes: a last-bit change of exp/log
# alone moves them by 7e-9 (NumPy's against libm's, the float64 reference against the C restatement), so two float64 solves
# of the same lane are two draws of that noise and a per-lane ratio means nothing.  They are held as a population: the max
# of a set's stiff lanes within STIFF_FACTOR x the restatement's max over ALL stiff lanes of the model (stiff set and mixed
# wave), the stiff set's median within STIFF_FACTOR x the restatement's median there, and under STIFF_CAP.  Measured: max
# ratio 2.5 on the stiff sets, 7.4 on the two lanes of a mixed wave against the pooled max (n2000 d=3 init); median ratio
# at most 1.0 on the stiff sets; n4000's stiff set
# 2.44e-6, the restatement's own 2.44e-6.
STIFF_FACTOR, STIFF_CAP = 10.0, 1e-5
# V (init_dp_kernel): a forward difference — relative step 1e-6 for d = 1 (Vstart), 1e-4 for d = 3 (V = W M^-1 W, every entry
# over sqrt(V_pp V_rr), test_three_parameter_chains' normalisation) — against the same init of extended solves
# (tests/init_extended.py).  Non-stiff, non-adjacent lanes only (on stiff lanes the difference is the rounding noise above,
# times 1e6: 3e-3 for the restatement).  Measured, d = 1: ratio at most 1.2, max 7.7e-6 (nondefault mixed; the restatement
# 7.7e-6 too).  d = 3 (this test's box, width 1 in a and b): ratio at most 1.1 (max and median), max 4.2e-6 (n2000
# mixed; the restatement 3.9e-6 there): the cap leaves 4.7x.
FACTOR_V = 4.0
V_FLOOR = {1: 1e-9, 3: 1e-9}
V_CAP = {1: 2e-5, 3: 2e-5}
INIT_FD = {1: 1e-6, 3: 1e-4}
PARITY = 1e-9

_PROBLEMS, _ORACLE = {}, {}


def _problem(oracle_mod, name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = X.Problem(oracle_mod.ModelSpec, name)
    return _PROBLEMS[name]


def _oracle(cpu_engine, p, variant):
    """the C restatement on problem p: (ssq, acc, per-lane errors against the reference), cached"""
    key = (p.name, variant)
    if key not in _ORACLE:
        assert cpu_engine.set_model(p.m, 1) == p.data.size
        ssq, acc = p.forward(cpu_engine, variant)
        _ORACLE[key] = (ssq, acc) + X.rel_errors(acc, ssq, *p.ext[variant])
    return _ORACLE[key]


def _stiff(p, variant, s):
    rec, sl = p.rec[variant], p.lanes(s)
    return ((rec.rejects[:, sl].sum(axis=0) > 0) | (rec.steps[2:, sl].max(axis=0) > 1)) & (rec.failed_at[sl] < 0)


def _check(tag, g, o, factor, floor, cap, fails):
    """g, o: per-lane errors of GPU and restatement on the lanes of one set that are held to the reference"""
    if g.size == 0:
        return
    gm, gd, om, od = g.max(), np.median(g), o.max(), np.median(o)
    print(f"{tag}: gpu max {gm:.2e} med {gd:.2e} | oracle max {om:.2e} med {od:.2e} | ratio max {gm / max(om, floor):.1f} "
          f"med {gd / max(od, floor):.1f}")
    if not (gm <= factor * max(om, floor) and gd <= factor * max(od, floor) and gm < cap):
        fails.append(tag)


def _held(p, variant, s, g_traj, g_ssq, o_traj, o_ssq, tag, fails, ssq_only=False):
    """one set: the lanes held to the reference (not adjacent, not failing, not stiff), the stiff ones to STIFF_CAP"""
    sl = p.lanes(s)
    rec = p.rec[variant]
    adj, fail, st = rec.adjacent[sl], rec.failed_at[sl] >= 0, _stiff(p, variant, s)
    keep = ~adj & ~fail & ~st
    if not ssq_only:
        _check(f"{tag} traj", g_traj[sl][keep], o_traj[sl][keep], FACTOR_TRAJ, TRAJ_FLOOR, TRAJ_CAP, fails)
    _check(f"{tag} ssq", g_ssq[sl][keep], o_ssq[sl][keep], FACTOR_SSQ, SSQ_FLOOR, SSQ_CAP, fails)
    if st.any():
        g, o = (g_ssq, o_ssq) if ssq_only else (g_traj, o_traj)
        pooled = np.concatenate([o[p.lanes(t)][_stiff(p, variant, t) & ~rec.adjacent[p.lanes(t)]] for t in ("stiff", "mixed")])
        gs, os_ = g[sl][st & ~adj], o[sl][st & ~adj]
        if gs.size:
            gm, om, pm = gs.max(), os_.max(), pooled.max()
            print(f"{tag} stiff lanes ({gs.size}): gpu max {gm:.2e} med {np.median(gs):.2e} | oracle max {om:.2e} "
                  f"med {np.median(os_):.2e} pooled max {pm:.2e} | ratio max {gm / pm:.1f} (same lanes {gm / om:.1f}) "
                  f"med {np.median(gs) / np.median(os_):.1f}")
            ok = gm <= STIFF_FACTOR * pm and gm < STIFF_CAP
            if gs.size >= 16:
                ok = ok and np.median(gs) <= STIFF_FACTOR * np.median(os_)
            if not ok:
                fails.append(f"{tag} stiff")
    return adj


@pytest.mark.parametrize("name", list(X.CASES))
def test_forward_dop853_within_float64_rounding(gpu_engine, cpu_engine, oracle_mod, name):
    """The forward kernel (trajectory and SSq) on every lane set, with and without per-lane (a, b)."""
    p = _problem(oracle_mod, name)
    fails, n_adj = [], 0
    for variant in p.variants:
        o_ssq, o_acc, ot, os_ = _oracle(cpu_engine, p, variant)
        assert gpu_engine.set_model(p.m, 1) == p.data.size
        ssq, acc = p.forward(gpu_engine, variant)
        gt, gs = X.rel_errors(acc, ssq, *p.ext[variant])
        for s in p.sets:
            adj = _held(p, variant, s, gt, gs, ot, os_, f"{name} {variant} {s}", fails)
            sl = p.lanes(s)
            n_adj += int(adj.sum())
            # decision-adjacent lanes: today's parity tolerance against the restatement
            for i in np.flatnonzero(adj):
                j = sl.start + i
                e = np.abs(acc[:, j] - o_acc[:, j]).max() / np.abs(o_acc[:, j]).max()
                print(f"{name} {variant} {s} adjacent lane {i}: gpu vs restatement {e:.1e}")
                if not (e < PARITY or _stiff(p, variant, s)[i]):
                    fails.append(f"{name} {variant} {s} adjacent {i}")
            for i in np.flatnonzero(p.rec[variant].failed_at[sl] >= 0):  # zeros after the failing call
                k = p.rec[variant].failed_at[sl][i]
                if not (acc[k + 1:, sl.start + i] == 0).all():
                    fails.append(f"{name} {variant} {s} failed lane {i}")
    print(f"{name}: {n_adj} decision-adjacent lanes")
    assert not fails, fails


SAMPLER_CASES = ["n500", "nondefault", "n2000"]
SAMPLER_SETS = ("fast", "fast_edge", "guard_trip", "mixed", "stiff")


def _rel(g, ref):
    return (np.abs(np.asarray(g, np.float64).astype(X.LD) - ref) / np.abs(ref)).astype(np.float64)


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("name", SAMPLER_CASES)
def test_sampler_and_init_dop853_within_float64_rounding(gpu_engine, cpu_engine, oracle_mod, name, d):
    """init_dp_kernel's ssq0, std2_0 and (d = 1) Vstart, and the sampler's own solve, one iteration with forced acceptance
    (proposal covariance (1e-7 q)^2, sigma^2 = 1e300) through mcmc_run (Philox: get_state()'s SSq against the reference at
    the proposal it made) and mcmc_replay (z = 0: the start point itself) — against the reference, to the forward test's
    tolerance.  d = 1: q = Dc with the model's (a, b); d = 3: q = (Dc, a, b) with the "ab" variant's b."""
    p = _problem(oracle_mod, name)
    variant = "plain" if d == 1 else "ab"
    if variant not in p.variants:
        pytest.skip(f"{name} has no (a, b) variant")
    _, _, ot, os_ = _oracle(cpu_engine, p, variant)
    gpu_engine.set_model(p.m, 1)
    cpu_engine.set_model(p.m, 1)
    fails, runs = [], {}
    N, C, L = p.data.size, X.WAVE, p.dc.size

    def held(s, g_set, what):
        full = np.zeros(L)
        full[p.lanes(s)] = g_set
        _held(p, variant, s, None, full, ot, os_, f"{name} d={d} {s} {what}", fails, ssq_only=True)

    for s in SAMPLER_SETS:
        sl = p.lanes(s)
        q0 = p.dc[sl].reshape(C, 1) if d == 1 else np.stack([p.dc[sl], p.a[variant][sl], p.b[variant][sl]], axis=1)
        lo, hi = [0.0] * d, [100.0 * p.dc.max()] + [1.0] * (d - 1)
        gpu_engine.mcmc_init(q0, p.data, lo, hi, seed=17, prior_len=3, fd_rel_step=INIT_FD[d])
        _, ssq0, std20, V0 = gpu_engine.get_state()
        ext = p.ext[variant][1][sl]
        held(s, _rel(ssq0, ext), "init ssq0")
        held(s, _rel(std20, ext / (N - 3)), "init std2_0")
        # the proposal covariance against the extended init (tests/init_extended.py) at the same forward-difference step
        cpu_engine.mcmc_init(q0, p.data, lo, hi, seed=17, prior_len=3, fd_rel_step=INIT_FD[d])
        Vc = cpu_engine.get_state()[3]
        vext = I.initial_state_ext(X.solve, p.m, q0, p.data, INIT_FD[d], 3, lo, hi, acc0=p.ext[variant][0][:, sl])[2]
        keep = ~p.rec[variant].adjacent[sl] & ~_stiff(p, variant, s)
        gv, ov = I.v_errors(V0, vext), I.v_errors(Vc, vext)
        what = "Vstart" if d == 1 else "V"
        if keep.any():
            _check(f"{name} d={d} {s} init {what}", gv[keep], ov[keep], FACTOR_V, V_FLOOR[d], V_CAP[d], fails)
        if (~keep).any():
            print(f"{name} d={d} {s} init {what}, stiff/adjacent lanes: gpu max {gv[~keep].max():.1e} oracle max {ov[~keep].max():.1e}")
        V = np.zeros((C, d, d))
        for k in range(d):
            V[:, k, k] = (1e-7 * q0[:, k]) ** 2
        for replay in (False, True):
            gpu_engine.set_state(q=q0, V=V, std2=np.full(C, 1e300))
            if replay:
                tq, _, ta = gpu_engine.mcmc_replay(np.zeros((1, C, d)), np.full((1, C), 1e-300), np.full((1, C), 250.0))
            else:
                tq, _, ta = gpu_engine.mcmc_run(1)
            assert np.asarray(ta[0]).all(), (name, s, d, replay)
            runs[(s, replay)] = (np.array(tq[0]), np.asarray(gpu_engine.get_state()[1], np.float64))
        held(s, _rel(runs[(s, True)][1], ext), "replay ssq")
    # the extended SSq at the Philox proposals (one solve over every set)
    qr = np.concatenate([runs[(s, False)][0] for s in SAMPLER_SETS])
    _, ssq_run, _ = X.solve(p.m, qr[:, 0], qr[:, 1] if d == 3 else None, qr[:, 2] if d == 3 else None, data=p.data)
    for i, s in enumerate(SAMPLER_SETS):
        held(s, _rel(runs[(s, False)][1], ssq_run[C * i:C * (i + 1)]), "run ssq")
    assert not fails, fails
