"""
The specification of the sampler with the stiffness among the parameters (tests/kstiff_reference.py, tests/kstiff_cases.py).  No GPU.
  1. A lane with its own k among lanes with other k is that lane solved alone with the scalar k, bit for bit.
  2. The "why" table: a stiffness fixed 20 % off moves the best Dc, by >= 0.5 under the step history and by >= 3 under the hold.
  3. What the data determine: the Laplace SDs and the condition numbers at the truth, d = 4 and d = 2, step and hold.
  4. The d = 2 yardstick: the tensor Simpson quadrature at two resolutions, and the weight on its window's edge.
  5. The d = 4 yardstick: self-normalised importance sampling, with its three conditions.
  6. The closed form at d = 4: two resolutions of its quadrature agree, and its exact draws pass its own check.
"""
import numpy as np
import pytest

import kstiff_cases as KC
import kstiff_reference as KR
import law_cases as C
import law_reference as R
import observe_reference as O
import posterior_reference as P
import stiff_cases as SC
import stiff_reference as S


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


@pytest.mark.parametrize("history", ("step", "hold"))
@pytest.mark.parametrize("law", R.LAWS)
def test_a_lane_with_its_own_k_is_that_lane_alone(law, history):
    m = C.spec()
    vl = R.table(m, history)
    rng = np.random.default_rng(3)
    n = 9
    pts = np.column_stack([rng.uniform(10.0, 60.0, n), rng.uniform(0.0105, 0.0115, n), rng.uniform(0.0135, 0.0145, n), rng.uniform(2e-3, 6e-3, n)])
    both = KR.trajectory_lane(m, pts, vl, law)
    data = both["mu"][:, 0] + 1e-3
    ssq = KR.forward_lane(m, pts, vl, law, "mu", data)[1]
    for i in range(n):
        alone = S.trajectory_lane(m, float(pts[i, 3]), [pts[i, 0]], vl, law, [pts[i, 1]], [pts[i, 2]])
        for obs in O.OBSERVABLES:
            assert np.isfinite(alone[obs]).all() and np.array_equal(_bits(both[obs][:, i]), _bits(alone[obs][:, 0])), (obs, i)
        # the SSq too, bit for bit (added sample by sample) — and it is stiff_reference.forward_lane's to rounding, whose sum is NumPy's
        assert _bits(ssq[i]) == _bits(KR.forward_lane(m, pts[i], vl, law, "mu", data)[1][0]), i
        assert _bits(ssq[i]) == _bits(KR.ssq_in_order(alone["mu"], data)[0]), i
        one = S.forward_lane(m, float(pts[i, 3]), [pts[i, 0]], vl, law, "mu", [pts[i, 1]], [pts[i, 2]], data)[1][0]
        assert abs(ssq[i] - one) <= 1e-13 * one
    # d = 2 is d = 4 with the model's (a, b)
    two = KR.trajectory_lane(m, pts[:, [0, 3]], vl, law)
    four = KR.trajectory_lane(m, np.column_stack([pts[:, 0], np.full(n, m.a), np.full(n, m.b), pts[:, 3]]), vl, law)
    assert np.array_equal(_bits(two["mu"]), _bits(four["mu"]))
    with pytest.raises(ValueError, match="points are"):
        KR.columns(np.zeros((3, 3)))


@pytest.mark.parametrize("history, moves", [("step", 0.5), ("hold", 3.0)])
def test_a_wrong_fixed_stiffness_moves_dc(history, moves):
    """k fixed at 1.6e-3 and 2.4e-3 on data from k = 2e-3, Dc = 20: best Dc 19.0 and 21.0 (SSq 1.44 x and 1.37 x the floor) under the
    step history, 16.75 and 24.5 (3.3 x, 2.6 x) under the hold, when this was written."""
    w = KC.wrong_k(history)
    print(history, w)
    (lo_dc, lo_r), (hi_dc, hi_r) = w[0.8], w[1.2]
    assert lo_dc <= R.BF_TRUTH - moves and hi_dc >= R.BF_TRUTH + moves
    assert lo_r > 1.2 and hi_r > 1.2


def test_what_the_data_determine():
    """At the truth under the step history every one of (Dc, a, b, k) is determined to 0.5 - 2 % (both laws); under the hold history the
    four-parameter problem is nearly degenerate (the SD of Dc is of the order of Dc, the condition number in the hundreds); (Dc, k)
    alone is determined to 0.5 - 2.5 % under both."""
    for law in R.LAWS:
        p = KC.problem4(law)
        rel = p["truth_sd"] / KC.truth(p["m"], 4)
        print(f"step {law}: SDs {100 * rel} %, condition number {p['truth_cond']:.1f}; least-squares point {p['q']}")
        assert (rel > 0.003).all() and (rel < 0.025).all() and p["truth_cond"] < 20.0
        # the figures MCMC.sample_stiffness's docstring and DESIGN 4u quote, to 3 % of each
        quoted = {"aging": ([1.156, 0.864, 0.564, 1.457], 7.32), "slip": ([1.560, 1.051, 0.688, 1.402], 8.49)}[law]
        assert np.allclose(100 * rel, quoted[0], rtol=0.03) and abs(p["truth_cond"] / quoted[1] - 1.0) < 0.03
        assert (np.abs(p["q"] - KC.truth(p["m"], 4)) < 4.0 * p["sd"]).all()
    h = SC.why_problem("hold")
    t = KC.truth(h["m"], 4)
    J, _, ssq = KR.normal(h["m"], h["vl"], "aging", KC.OBS, t, h["data"])
    _, sd, cond = KR.laplace(J, ssq, h["data"].size)
    print(f"hold aging: SDs {100 * sd / t} %, condition number {cond:.0f}")
    assert sd[0] / t[0] > 0.5 and cond > 100.0
    assert np.allclose(100 * sd / t, [101.0, 7.52, 50.4, 1.674], rtol=0.03) and abs(cond / 160.0 - 1.0) < 0.03  # the docstring's figures
    for history in ("step", "hold"):
        p = KC.problem2(history)
        print(f"{history} d = 2: least-squares point {p['q']}, SDs {100 * p['sd'] / p['q']} %, condition number {p['cond']:.1f}")
        assert (p["sd"] / p["q"] > 0.005).all() and (p["sd"] / p["q"] < 0.025).all() and p["cond"] < 5.0
        quoted = {"step": ([0.692, 1.412], 1.73), "hold": ([1.542, 0.640], 1.52)}[history]  # "0.6-1.6 %, condition number below 2"
        assert np.allclose(100 * p["sd"] / p["q"], quoted[0], rtol=0.03) and abs(p["cond"] / quoted[1] - 1.0) < 0.03


@pytest.mark.parametrize("history", ("step", "hold"))
def test_quadrature_yardstick(history):
    """65 x 33 against 129 x 65 nodes over +-8 Laplace SDs about the least-squares point: both means agree to 1e-6 relative (5e-11
    when this was written) and the largest weight on the window's edge is <= 1e-4 of the peak (5e-12); the window lies inside the box.
    The hold history's means were 20.80897 and 2.006727e-3."""
    p = KC.problem2(history)
    coarse, fine = KC.yardstick2(history, n=(65, 33)), KC.yardstick2(history)
    rel = np.abs(coarse["mean"] / fine["mean"] - 1.0)
    print(f"{history}: means {fine['mean']}, SDs {fine['sd']}; 65 x 33 against 129 x 65 {rel}; edge {fine['edge']:.1e}")
    assert (rel < 1e-6).all() and (np.abs(coarse["sd"] / fine["sd"] - 1.0) < 1e-5).all()
    assert fine["edge"] <= 1e-4 and coarse["edge"] <= 1e-4
    assert fine["x"][0] > p["lo"][0] and fine["x"][-1] < p["hi"][0] and fine["y"][0] > p["lo"][1] and fine["y"][-1] < p["hi"][1]
    if history == "hold":
        assert abs(fine["mean"][0] - 20.80897) < 1e-4 and abs(fine["mean"][1] - 2.006727e-3) < 1e-8


@pytest.mark.parametrize("law", R.LAWS)
def test_importance_yardstick(law):
    """16 384 draws of the t5 with 1.5^2 x the Laplace covariance: every draw inside the box and finite, ESS >= 0.25 n, the largest
    normalised weight <= 1e-3 (ESS / n 0.49, weight 2.2e-4, standard error 0.0094 posterior SD per parameter when this was written)."""
    y = KC.problem4(law)["yard"]
    print(f"{law}: mean {y['mean']}, SD {y['sd']}, SE / SD {y['se'] / y['sd']}, ESS / n {y['ess'] / KC.IS_N:.3f}, largest weight {y['wmax']:.2e}")
    assert y["inbox"] and y["finite"]
    assert y["ess"] >= 0.25 * KC.IS_N and y["wmax"] <= 1e-3
    assert (y["se"] < 0.02 * y["sd"]).all()


def test_closed_form_at_four_parameters():
    ref = KC.closed4()
    assert ref.outside < 1e-6
    c = KC.CLOSED4
    assert np.linalg.eigvalsh(np.array(c["K"])).min() > 0 and c["lo"][3] > 0
    coarse = KC.Closed4(n=(40, 20, 20, 20))
    for name in KC.NAMES4:
        a, b = ref.marg[name], coarse.marg[name]
        # check4 at 262 144 chains resolves a mean to 4.5 / 512 = 9e-3 SD and a variance to ~1e-2 of itself: the grid is held to 1e-3 of that
        assert abs(a.mean - b.mean) < 1e-5 * a.sd and abs(a.var / b.var - 1.0) < 1e-5 and abs(a.kurt - b.kurt) < 1e-4, name
    # the box cuts: the fourth parameter's mean lies below its centre, its upper face 0.7 SD of the uncut density above it
    assert ref.marg["k"].mean < c["q0"][3] - 0.03
    rng = np.random.default_rng(KC.SEED4)
    q = ref.draw(rng, 65536)
    assert ((q > c["lo"]) & (q < c["hi"])).all()
    fails = []
    KC.check4("exact draws", ref, q, P.draw_std2(rng, ref.fn(*q.T), c["shape"]), fails)
    assert not fails, fails
    # ... and the check sees a wrong target: the draws of the uncut density's own scale, 5 % wider
    wide = np.array(c["q0"]) + 1.05 * (q - np.array(c["q0"]))
    bad = []
    KC.check4("5 % wider", ref, wide, P.draw_std2(rng, ref.fn(*q.T), c["shape"]), bad)
    assert bad
