"""
CPU tests of the extended-precision DOP853 reference (tests/dop853_extended.py) and of the float64 CPU restatement against it.

The reference is pinned to the reference project's own trajectories (the golden dop853 vectors) and, run in float64, to the
C restatement (the same algorithm).  The restatement's distance from it — the rounding error of a plain float64 DOP853 — is
measured on the lane sets and models the GPU tests use (tests/test_gpu_dop853_extended.py), where it is the yardstick the
kernels are held to; and each set's record shows the path it was placed on.
"""
import numpy as np
import pytest

import dop853_extended as X

CPU_CASES = [n for n, c in X.CASES.items() if c[3]]

# The C restatement against the extended reference over every CPU case, set and variant, decision-adjacent lanes excluded.
# Measured: trajectory max 2.9e-11 (fast lanes at the largest Dc, n500_mu+5e-4: their acc is a small part of V, so V's own
# rounding, 1e-16 per interval, is a 1e-11 part of it; 3.4e-13 and below on the fast_edge and guard_trip sets), SSq max
# 3.2e-12.  The caps leave ~3x.
ORACLE_TRAJ_CAP, ORACLE_SSQ_CAP = 1e-10, 1e-11
# stiff lanes (the stiff set, the mixed wave's two): hundreds of adaptive steps whose sizes feed back into the solution and
# amplify rounding; measured trajectory max 4.5e-7 (vref_si; 7.4e-9 and below on the other models) against the reference —
# the bound test_dop853_mode_matches_oracle_and_reference gives Dc = 1 for the same reason
STIFF_CAP = 1e-6

_PROBLEMS = {}


def problem(oracle_mod, name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = X.Problem(oracle_mod.ModelSpec, name)
    return _PROBLEMS[name]


def stiff_lanes(p, s):
    """lanes of set s whose path includes adaptive steps (the stiff set, the mixed wave's stiff lanes)"""
    rec = p.rec["plain"]
    sl = p.lanes(s)
    return ((rec.rejects[:, sl].sum(axis=0) > 0) | (rec.steps[2:, sl].max(axis=0) > 1)) & (rec.failed_at[sl] < 0)


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).nmant >= 63
    assert np.longdouble(1) + np.longdouble(2.0 ** -62) != np.longdouble(1)


def test_tableau_is_the_compiled_one():
    """parsed from include/rsf_dop853_tableau.h: row sums = nodes, B sums to 1, the estimators annihilate constants"""
    np.testing.assert_allclose(X.TAB_A.sum(axis=1), X.TAB_C[1:], rtol=0, atol=1e-15)
    assert abs(X.TAB_B.sum() - 1) < 1e-15 and abs(X.TAB_E5.sum()) < 1e-15 and abs(X.TAB_E3.sum()) < 1e-15


def test_reference_matches_the_reference_projects_dop853(oracle_mod, golden, cpu_engine):
    """The golden trajectories of the reference project (SciPy's dop853): the extended reference is as close to them as the
    C restatement is, or — where the restatement is bit-identical to them, most cases — within the float64 rounding of a
    DOP853 solve (measured 4.6e-12, n2000_dc5000); Dc = 1, the stiff case, to its own bound."""
    g, meta = golden.npz("forward"), golden.json("forward")
    for case in meta["cases"]:
        m = oracle_mod.ModelSpec(case["nsteps"])
        m.RadiationDamping, m.a, m.b, m.integrator = case["damping"], case["a"], case["b"], "dop853"
        acc, _, rec = X.solve(m, [case["dc"]])
        assert cpu_engine.set_model(m, 1) == m.nout
        _, ac = cpu_engine.forward([case["dc"]])
        ref = g[case["tag"]]
        scale = np.abs(ref).max()
        e_ext = np.abs(acc[:, 0].astype(np.float64) - ref).max() / scale
        e_c = np.abs(ac[:, 0] - ref).max() / scale
        print(f"{case['tag']:26s} extended {e_ext:.1e}  C restatement {e_c:.1e}  adjacent {bool(rec.adjacent[0])}")
        if case["dc"] < 10:
            assert e_ext < 1e-6, case["tag"]  # (test_dop853_mode_matches_oracle_and_reference's bound for Dc = 1)
        else:
            assert e_ext <= max(3 * e_c, 1e-11), (case["tag"], e_ext, e_c)


def test_float64_mode_is_the_c_restatement(oracle_mod, cpu_engine):
    """dtype=float64 (with the C library's exp/log/sin/pow, as the restatement calls them): the same algorithm in the same
    arithmetic — bit for bit, on every lane of every set: the stiff lanes' rejections and short steps, the failed call."""
    p = problem(oracle_mod, "n500")
    assert cpu_engine.set_model(p.m, 1) == p.data.size
    ssq_c, acc_c = p.forward(cpu_engine, "plain")
    acc, ssq, rec = X.solve(p.m, p.dc, p.a["plain"], p.b["plain"], data=p.data, dtype=np.float64)
    np.testing.assert_array_equal(acc, acc_c)
    np.testing.assert_allclose(ssq, ssq_c, rtol=1e-14)  # (NumPy sums the squares pairwise, the restatement in order)
    # the extended reference takes the same decisions on every lane but the adjacent, stiff and failing ones (a stiff lane
    # amplifies rounding until a later decision may flip: counted, not asserted)
    loose = p.rec["plain"].adjacent | (p.rec["plain"].failed_at >= 0)
    loose |= np.concatenate([stiff_lanes(p, s) for s in p.sets])
    for k in ("steps", "rejects", "one_step"):
        same = (getattr(rec, k) == getattr(p.rec["plain"], k)).all(axis=0)
        print(f"decisions {k}: differ on {int((~same).sum())} lanes, of which stiff/adjacent/failing {int((~same & loose).sum())}")
        assert (same | loose).all(), k
    np.testing.assert_array_equal(rec.failed_at, p.rec["plain"].failed_at)


@pytest.mark.parametrize("name", CPU_CASES)
def test_c_restatement_is_within_float64_rounding_of_the_reference(cpu_engine, oracle_mod, name):
    """The float64 C restatement against the extended reference, set by set: the size the GPU tests compare the kernels'
    error with."""
    p = problem(oracle_mod, name)
    assert cpu_engine.set_model(p.m, 1) == p.data.size
    worst_t, worst_s, worst_st = [], [], []
    for variant in p.variants:
        ssq, acc = p.forward(cpu_engine, variant)
        traj, serr = X.rel_errors(acc, ssq, *p.ext[variant])
        adj = p.rec[variant].adjacent
        fail = p.rec[variant].failed_at >= 0
        for s in p.sets:
            sl = p.lanes(s)
            st = stiff_lanes(p, s)
            keep = ~adj[sl] & ~fail[sl] & ~st
            print(f"{name:14s} {variant:5s} {s:10s} traj max {traj[sl][keep].max(initial=0):.1e}  "
                  f"ssq max {serr[sl][keep].max(initial=0):.1e}  stiff traj max {traj[sl][st & ~adj[sl]].max(initial=0):.1e}  "
                  f"adjacent {int(adj[sl].sum())}")
            worst_t.append((traj[sl][keep].max(initial=0), variant, s))
            worst_s.append((serr[sl][keep].max(initial=0), variant, s))
            if st.any():
                worst_st.append((traj[sl][st & ~adj[sl]].max(initial=0), variant, s))
            # a failed lane: zeros after its failing call, as in the restatement
            for i in np.flatnonzero(fail[sl]):
                k = p.rec[variant].failed_at[sl][i]
                assert (acc[k + 1:, sl][:, i] == 0).all() and (p.ext[variant][0][k + 1:, sl][:, i] == 0).all()
    assert max(worst_t)[0] < ORACLE_TRAJ_CAP, max(worst_t)
    assert max(worst_s)[0] < ORACLE_SSQ_CAP, max(worst_s)
    assert not worst_st or max(worst_st)[0] < STIFF_CAP, max(worst_st)


@pytest.mark.parametrize("name", CPU_CASES)
def test_lane_sets_take_their_paths(oracle_mod, name):
    """Each set's record shows the path it was placed on; decision-adjacent lanes are a small minority."""
    p = problem(oracle_mod, name)
    k0 = X.placement_from(p.m)
    for variant in p.variants:
        rec = p.rec[variant]
        frac = rec.guard_frac(k0)
        for s in p.sets:
            sl = p.lanes(s)
            steady, f, adj = rec.steady[sl], frac[sl], rec.adjacent[sl]
            rej = rec.rejects[:, sl].sum(axis=0) > 0
            multi = rec.steps[2:, sl].max(axis=0) > 1
            tag = (name, variant, s)
            assert adj.sum() <= 3, tag
            if variant == "ab":  # same Dc, b moved by up to 0.002: the sets keep their paths (guard fractions move a little)
                if s in ("fast", "fast_edge", "guard_trip"):
                    assert steady.all(), tag
                elif s == "mixed":
                    st = np.zeros(X.WAVE, bool)
                    st[list(X.MIXED_STIFF)] = True
                    assert steady[~st].all() and not steady[st].any() and (rej | multi)[st].all(), tag
                elif s == "stiff":
                    assert not steady.any() and multi.all() and rej.mean() > 0.8, tag
                elif s == "failed":
                    fa = rec.failed_at[sl]
                    assert (fa >= 0).sum() == 1 and fa[3] == 1 and np.delete(steady, 3).all(), tag
                continue
            if s == "fast":
                assert steady.all() and f.max() < 0.35, tag
            elif s == "fast_edge":
                assert steady.all() and 0.5 <= f.min() and f.max() < 0.95, tag
            elif s == "guard_trip":
                assert steady.all() and f.min() > 1.5, tag
            elif s == "mixed":
                st = np.zeros(X.WAVE, bool)
                st[list(X.MIXED_STIFF)] = True
                assert steady[~st].all() and not steady[st].any() and (rej | multi)[st].all(), tag
            elif s == "stiff":
                assert not steady.any() and multi.all() and rej.mean() > 0.8, tag
                hc_short = (rec.steps[2:, sl] > 1).any(axis=0)  # short predicted steps: intervals of several steps
                assert hc_short.all(), tag
            elif s == "failed":
                fa = rec.failed_at[sl]
                assert (fa >= 0).sum() == 1 and fa[3] == 1, tag  # the one lane fails in its first call (a sample, then zeros)
                assert np.delete(steady, 3).all(), tag
