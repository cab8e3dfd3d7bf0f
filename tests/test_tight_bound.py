"""
The a-priori bound that lets a TIGHT trip of the float64 sampler run without its guard (csrc/rsf_device.h, tight_needs_guard),
restated in tests/tight_bound.py and held against the extended-precision RK4 of tests/rk4_extended.py.  No GPU.

Soundness   wherever the bound says that a 16-step trip needs no guard, each of the four maxima the guard would have measured
            in that trip — in extended precision — lies below 0.95 x its threshold.  The bound proves 0.9 x in exact
            arithmetic (the derivation stands next to tight_needs_guard); 0.95 leaves room for nothing but float64 rounding.
Usefulness  with the default a, b and the built-in loading it says so for EVERY trip of the 50 s series at h = 0.025,
            Dc in [500, 1500], and at h = 0.0125, Dc in [600, 1500] — the shapes of the benchmark's headline and of its
            three-parameter shard; at h = 0.1 it does from Dc = 2000 up.
Grid: Dc log-spaced 150 .. 1e4; (a, b) in {(0.011, 0.014), (0.03, 0.034), (0.008, 0.022)}; h in {0.1, 0.025, 0.0125}; radiation
damping on, off and with k1 10^4 times the default; the built-in loading, a constant 10 V_ref and a caller's oscillating
table (the latter two at h = 0.1 and 0.025, damping on).
"""
import numpy as np
import pytest

import rk4_extended as X
import tight_bound as T

AB = ((0.011, 0.014), (0.03, 0.034), (0.008, 0.022))
DC = np.geomspace(150.0, 1.0e4, 20)
DAMPING = {"damped": {}, "undamped": {"RadiationDamping": False}, "k1_large": {"k1": 1.0e-3}}
NSTEPS = {0.1: 500, 0.025: 2000, 0.0125: 4000}  # the 50 s series


def _oscillating(m, t):
    return m.V_ref * (2.0 + 1.5 * np.cos(3.0 * t) * np.exp(-t / 40))  # in [0.5, 3.5] V_ref: a caller's table, not the built-in range


LOADINGS = {"builtin": None, "constant": lambda m, t: np.full(t.shape, 10.0 * m.V_ref), "oscillating": _oscillating}


def _lanes():
    dc = np.tile(DC, len(AB))
    a = np.repeat([p[0] for p in AB], DC.size)
    b = np.repeat([p[1] for p in AB], DC.size)
    return dc, a, b


def _scan(oracle_mod, h, damping, loading):
    n = NSTEPS[h]
    m = oracle_mod.ModelSpec(n, 0.0, 50.0, 1)
    for k, v in DAMPING[damping].items():
        setattr(m, k, v)
    assert m.delta_t == h
    dc, a, b = _lanes()
    vl = None
    if LOADINGS[loading] is not None:
        t = float(m.t_start) + np.arange(2 * (m.nout - 1) + 1, dtype=np.float64) * (0.5 * h)
        vl = LOADINGS[loading](m, t)
    return T.scan(m, dc, m.nout - 1, a=a, b=b, vl=vl)


def _check_sound(tag, r):
    ok = ~r["need"]
    print(f"{tag}: {r['need'].shape[0]} trips x {r['need'].shape[1]} lanes, the bound frees {ok.mean():.3f} of them")
    for k, thr in T.GUARDS.items():
        rel = r[k] / thr
        worst = rel[ok].max() if ok.any() else 0.0
        print(f"  {k:6s} largest maximum over its threshold: {worst:.3f} where the bound says yes, {rel[~ok].max() if (~ok).any() else 0.0:.3f} where it says no")
        assert worst < 0.95, f"{tag}: the bound let through a trip whose {k} reaches {worst:.3f} of its guard"
    return ok


@pytest.mark.parametrize("damping", list(DAMPING))
@pytest.mark.parametrize("h", [0.1, 0.025, 0.0125])
def test_bound_is_sound_and_useful_builtin_loading(oracle_mod, h, damping):
    r = _scan(oracle_mod, h, damping, "builtin")
    ok = _check_sound(f"h {h} {damping}", r)
    # not vacuous either way: it frees trips, and it refuses the small-Dc lanes whose increments do leave the guard
    assert ok.any() and (~ok).any()
    left = np.maximum.reduce([r[k] / thr for k, thr in T.GUARDS.items()]) >= 1.0
    assert left.any() and not (left & ok).any()
    # usefulness: default a, b = the first block of lanes
    dc = DC
    first = ok[:, :DC.size]
    span = {0.025: (500.0, 1500.0), 0.0125: (600.0, 1500.0), 0.1: (2000.0, 1.0e4)}[h]
    sel = (dc >= span[0]) & (dc <= span[1])
    assert sel.sum() >= 3
    frees = first[:, sel].all(axis=0)
    print(f"  default a, b, Dc in {span}: trips freed per lane {first[:, sel].mean(axis=0)}; margins D / Dmax {r['D'][:, :DC.size][:, sel].max():.3f}, "
          f"rb / 0.9 B {r['rb'][:, :DC.size][:, sel].max():.3f}")
    if damping != "k1_large":
        assert frees.all(), f"h {h} {damping}: the bound keeps the guard on some trip of Dc = {dc[sel][~frees]}"


@pytest.mark.parametrize("loading", ["constant", "oscillating"])
@pytest.mark.parametrize("h", [0.1, 0.025])
def test_bound_is_sound_under_a_callers_loading(oracle_mod, h, loading):
    r = _scan(oracle_mod, h, "damped", loading)
    ok = _check_sound(f"h {h} {loading}", r)
    assert (~ok).any()  # a tenfold step in the loading, or a table beyond [0, 2 V_ref], is not waved through


def test_bound_needs_the_tables_own_range(oracle_mod):
    """given the built-in history's range for a table that leaves it, the bound would free trips it must not: the range is an
    input (rsf_set_loading computes the caller's), not a constant"""
    m = oracle_mod.ModelSpec(NSTEPS[0.025], 0.0, 50.0, 1)
    t = np.arange(2 * (m.nout - 1) + 1, dtype=np.float64) * (0.5 * m.delta_t)
    vl = np.full(t.shape, 10.0 * m.V_ref)
    dc = np.array([500.0, 1000.0])
    own = T.scan(m, dc, 64, vl=vl)
    wrong = T.scan(m, dc, 64, vl=vl, vl_range=(0.0, 2.0 * m.V_ref))
    rel = np.maximum.reduce([own[k] / thr for k, thr in T.GUARDS.items()])
    assert (rel[~own["need"]] < 0.95).all()
    assert own["need"][0].all()  # the first trip under the step: |V_l - v| = 9 V_ref
    assert (own["D"] > wrong["D"]).all()


def test_restated_rhs_is_rk4_extendeds(oracle_mod):
    m = oracle_mod.ModelSpec(500, 0.0, 50.0, 1)
    dc = X._w(np.array([300.0, 1000.0]))
    a, b = X._w(np.full(2, m.a)), X._w(np.full(2, m.b))
    mu, th = X._w(np.array([0.6, 0.601])), dc / X._w(m.V_ref) * X._w(1.01)
    t = X._w(0.3)
    V_l = X._w(m.V_ref) * (1 + np.exp(-t / 20) * np.sin(10 * t))
    for damping in (True, False):
        ref = X._rhs(t, mu, th, dc, a, b, X._w(m.V_ref), X._w(m.mu_ref), X._w(m.k1), damping)
        got = T._rhs_vl(V_l, mu, th, dc, a, b, X._w(m.V_ref), X._w(m.mu_ref), X._w(m.k1), damping)
        for x, y in zip(ref, got):
            assert np.array_equal(x, y)


def test_nan_inf_and_signs_keep_the_guard(oracle_mod):
    m = oracle_mod.ModelSpec(2000, 0.0, 50.0, 1)
    w, th = np.ones(6), np.full(6, 1000.0)
    dc, a, b = np.full(6, 1000.0), np.full(6, m.a), np.full(6, m.b)
    assert not T.needs_guard(w, th, m, dc, a, b, 0.0, 2.0)[0].any()  # the steady state at Dc = 1000, h = 0.025: no guard needed
    w[0], th[1], a[2] = np.nan, np.nan, np.nan
    w[3] = np.inf
    w[4] = -1.0   # a sign the derivation never assumed: |V_l - v| is then 3 V_ref, still far inside at this Dc
    dc[5] = -1000.0
    need = T.needs_guard(w, th, m, dc, a, b, 0.0, 2.0)[0]
    assert need[:4].all(), need
    assert T.needs_guard(w, th, m, dc, a, b, np.nan, 2.0)[0].all()
    assert T.predicted_unguarded(np.zeros((3, 64), bool)) == 48
    one = np.zeros((3, 64), bool)
    one[1, 7] = True
    alive = np.ones((3, 64), bool)
    assert T.predicted_unguarded(one) == 32
    alive[1:, 7] = False
    assert T.predicted_unguarded(one, alive) == 48
