"""
GPU tests of the state-law kernels (include/rsf_law.h, include/rsf_observe.h: rsf_law_forward / rsf_law_observe) against the
long-double specification BEYOND THE DEFAULT MODEL: the configuration matrix of tests/law_matrix_cases.py — per-lane (a, b), no
damping, k1 = 0, substeps > 1, a table in two chunks, V_ref != 1, mu_t_zero != mu_ref != 0.6, t_start != 0 — under the step and
the hold history and both laws:
  a. acc, mu, theta and velocity against long double by test_both_laws_against_long_double's rule, the yardstick floored at the
     default model's;
  b. the sum of squares at per-lane (a, b) and non-default attributes: the returned series' own, and the long-double one;
  c. the ageing-law acceleration of the tier kernels (rsf_forward_batch) under a custom history at V_ref != 1;
  d. a power of two for V_ref changes no bit of theta and mu, and of velocity and acc only the exponent;
  e. the front end on a non-default model.
The loading goes to the engine as a TABLE in the model's own units (law_reference.table scales by V_ref); every case is one
set_model and launches of one wave, the twelve lanes padded by law_cases.padded.
"""
import numpy as np
import pytest

import law_cases as C
import law_matrix_cases as M
import law_reference as R
import observe_reference as O

pytestmark = pytest.mark.gpu


def _model(pkg, m, table):
    """the package's model of the specification's attributes `m`, its loading `table`"""
    model = pkg.RateStateModel(number_time_steps=m.num_tsteps, start_time=m.t_start, end_time=m.t_final)
    for k in ("a", "b", "mu_ref", "V_ref", "k1", "mu_t_zero", "RadiationDamping", "substeps"):
        setattr(model, k, getattr(m, k))
    model.loading = table
    return model


def _arm(pkg, eng, s):
    """set_model of a solved entry; the table the engine holds is the specification's, at the specification's stage times"""
    eng.set_model(_model(pkg, s["m"], s["vl"]), s["m"].substeps)
    assert eng.nout == R.nout(s["m"])
    assert np.array_equal(eng.loading(), s["vl"]) and np.array_equal(eng.loading_times(), R.stage_times(s["m"]))


def _lanes(s):
    """-> (dc, a, b) of one wave: the entry's lanes, then law_cases.padded's Dc = 1000 IN THE ENTRY'S UNITS with the model's (a, b).
    (Dc = 1000 itself beside V_ref = 1e-6 is the default problem's Dc = 1e9: finite, but its V moves by 1e-9 of itself over the whole
    series and an acceleration differenced from it holds seven digits — the plain solve lay 1.2e-7 from the tiers there when this
    was written, the conditioning of that lane and no defect.)"""
    dc = C.padded(R.LANES) * s["factor"]
    assert np.array_equal(dc[:s["dc"].size], s["dc"])
    if s["a"] is None:
        return dc, None, None
    pad = dc.size - s["dc"].size
    return dc, np.concatenate([s["a"], np.full(pad, s["m"].a)]), np.concatenate([s["b"], np.full(pad, s["m"].b)])


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def _gate(tag, obs, got, s):
    """print and assert the project's rule for one series against long double"""
    n = s["dc"].size
    got = np.asarray(got)
    assert got.shape[0] == s["ext"][obs].shape[0] and np.isfinite(got).all(), (tag, obs)
    err, yard = M.error(obs, got[:, :n], s["ext"][obs]), s["yardstick"][obs]
    print(f"{tag} {obs}: GPU {err.max():.2e}, yardstick {yard:.2e} (own {s['own'][obs]:.2e}: specification {s['err_spec'][obs].max():.2e}, device "
          f"arrangement {s['err_lane'][obs].max():.2e}), ratio {err.max() / yard:.2f}; per lane against the device arrangement "
          f"{np.array2string(err / s['err_lane'][obs], precision=2)}")
    return obs, float(err.max()), yard


def _assert_gates(tag, gates):
    for obs, err, yard in gates:
        assert err < C.CAP, (tag, obs)
        assert err <= 4.0 * yard, (tag, obs)


# ---- a. the precision gate --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("name", M.NAMES)
def test_matrix_against_long_double(pkg, gpu_engine, name, law, history):
    """Per entry and observable the GPU's largest error against the long-double specification — relative to the lane's max|acc|
    for the acceleration, to the lane's excursion otherwise — is below law_cases.CAP and at most 4 x the yardstick: the larger of
    the two CPU float64 arrangements' largest error on the entry, floored at the default model's (the factor and its reason are
    test_both_laws_against_long_double's).  Measured on an MI355X when this was written: the largest ratio 1.44 (velocity,
    nondefault_sub3_ab, step history); DESIGN.md 4o holds the table."""
    s = M.solve(name, history, law)
    eng = gpu_engine
    _arm(pkg, eng, s)
    dc, a, b = _lanes(s)
    tag = f"{name} {history} {law}"
    gates = [_gate(tag, obs, eng.law_observe(law, obs, dc, a, b)[1], s) for obs in O.OBSERVABLES]
    _assert_gates(tag, gates)


# ---- b. the sum of squares ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("name", ["ab", "nondefault_sub3_ab", "chunks_ab"])
def test_matrix_ssq_is_the_returned_series_sum(pkg, gpu_engine, name, law):
    """test_ssq_is_the_returned_series_sum's two rules at per-lane (a, b), non-default attributes and a table in two chunks, every
    observable: SSq within 4 nout 2^-53 of the float64 sum of the RETURNED series' squared residuals, and within 1e-9 of the
    long-double specification's.  The data: the float64 specification's series of the Dc = 20 lane plus 5 % of its excursion."""
    s = M.solve(name, "step", law)
    eng = gpu_engine
    _arm(pkg, eng, s)
    dc, a, b = _lanes(s)
    n, lane = s["dc"].size, R.LANES.index(R.BF_TRUTH)
    for obs in O.OBSERVABLES:
        clean = s["spec"][obs][:, lane]
        data = clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(4).standard_normal(clean.size)
        ssq, series = eng.law_observe(law, obs, dc, a, b, data=data, want_ssq=True, want_series=True)
        ssq, series = np.asarray(ssq), np.asarray(series)
        own = ((series - data[:, None]) ** 2).sum(axis=0)
        ext = (((s["ext"][obs] - data.astype(R.LD)[:, None]) ** 2).sum(axis=0)).astype(np.float64)
        print(f"{name} {law} {obs}: SSq against its own series {np.abs(ssq / own - 1).max():.2e} (bound {4 * eng.nout * 2.0 ** -53:.2e}), against long "
              f"double {np.abs(ssq[:n] / ext - 1).max():.2e}")
        assert np.isfinite(ssq).all() and (ssq > 0).all(), obs
        assert (np.abs(ssq - own) <= 4 * eng.nout * 2.0 ** -53 * own).all(), obs
        assert (np.abs(ssq[:n] - ext) <= 1e-9 * ext).all(), obs
        # SSq alone is the same launch's
        assert np.array_equal(_bits(eng.law_observe(law, obs, dc, a, b, data=data, want_ssq=True, want_series=False)[0]), _bits(ssq)), obs


# ---- c. the tier kernels under a custom history at V_ref != 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("name", ["nondefault", "si"])
def test_tier_kernels_at_non_default_attributes(pkg, gpu_engine, name, history):
    """rsf_forward_batch — the incremental tiers on their custom-loading path — against law_forward's plain ageing-law solve
    within law_cases.CAP of the lane's max|acc|, and both against long double by rule (a)."""
    s = M.solve(name, history, "aging")
    eng = gpu_engine
    _arm(pkg, eng, s)
    dc, _, _ = _lanes(s)
    tiers, plain = np.asarray(eng.forward(dc)[1]), np.asarray(eng.law_forward("aging", dc)[1])
    tag = f"{name} {history}"
    gates = [_gate(tag + " tiers", "acc", tiers, s), _gate(tag + " plain", "acc", plain, s)]
    between = (np.abs(tiers - plain).max(axis=0) / np.abs(plain).max(axis=0)).max()
    print(f"{tag}: tiers against plain {between:.2e}")
    assert between < C.CAP
    _assert_gates(tag, gates)


# ---- d. exact unit scaling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("law", R.LAWS)
def test_a_power_of_two_for_v_ref_changes_no_bit(pkg, gpu_engine, law, history):
    """V_ref = 2^-20 with Dc, the table and 1 / k1 scaled along is the default problem with every velocity's exponent moved by
    20: theta and mu are the default model's series bit for bit, velocity and acc are after multiplication by 2^20 — unless a
    step of the device arithmetic (a reciprocal, say) is not homogeneous in V_ref.  The two CPU arrangements are bit-exact
    (tests/test_observe_reference.py).  Measured on an MI355X when this was written: bit-exact, every sample of every series
    under both laws and both histories — so bits are asserted."""
    one = M.solve("pow2", history, law)
    eng = gpu_engine
    got = {}
    default = {"m": C.spec(), "vl": R.table(C.spec(), history), "dc": np.asarray(R.LANES), "factor": 1.0, "a": None}
    for key, s in (("default", default), ("pow2", one)):
        _arm(pkg, eng, s)
        got[key] = {obs: np.asarray(eng.law_observe(law, obs, _lanes(s)[0])[1]) for obs in O.OBSERVABLES}  # the padding lanes too
    assert np.array_equal(one["vl"], default["vl"] * M.POW2) and np.array_equal(one["dc"], default["dc"] * M.POW2)
    worst = {}
    for obs in O.OBSERVABLES:
        want = got["default"][obs] * (M.POW2 if obs in ("acc", "velocity") else 1.0)  # exact: no series comes near the subnormals
        assert np.isfinite(want).all() and (np.abs(want[want != 0.0]) > 1e-280).all()
        ulps = np.abs(_bits(got["pow2"][obs]) - _bits(want))
        worst[obs] = int(ulps.max())
        print(f"{history} {law} {obs}: largest distance {worst[obs]} ulp, {int((ulps != 0).sum())} of {ulps.size} samples differ")
    for obs in O.OBSERVABLES:
        assert worst[obs] == 0, obs


# ---- e. the front end ----------------------------------------------------------------------------------------------------------------------
def test_front_end_on_a_non_default_model(pkg):
    """RateStateModel.trajectory(dc, a, b) and, with observable = 'theta', evaluate_batch(dc, a, b) on the non-default model at
    substeps 3 under the slip law and the step table: the four series within law_cases.CAP of long double."""
    s = M.solve("nondefault_sub3_ab", "step", "slip")
    model = _model(pkg, s["m"], s["vl"])
    model.state_law = "slip"
    try:
        out = model.trajectory(s["dc"], s["a"], s["b"])
        assert sorted(out) == sorted(O.OBSERVABLES)
        for obs in O.OBSERVABLES:
            assert out[obs].shape == (s["dc"].size, R.nout(s["m"]))
            err = M.error(obs, out[obs].T, s["ext"][obs]).max()
            print(f"trajectory {obs}: {err:.2e}")
            assert err < C.CAP, obs
        model.observable = "theta"
        batch = model.evaluate_batch(s["dc"], s["a"], s["b"])
        assert batch.shape == (s["dc"].size, R.nout(s["m"]))
        assert np.array_equal(_bits(batch), _bits(out["theta"]))
        assert M.error("theta", batch.T, s["ext"]["theta"]).max() < C.CAP
        t = model.time_axis()
        assert t[0] == s["m"].t_start and abs(t[-1] - (s["m"].t_start + (t.size - 1) * s["m"].delta_t)) < 1e-9
    finally:
        if model._engine is not None:
            model._engine.close()
