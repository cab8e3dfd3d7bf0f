"""
What tests/test_stiff_reference.py (CPU) and tests/test_gpu_stiff.py share (a test helper): the lane sets and data sets of the
state-law solve with a stiffness independent of Dc (tests/stiff_reference.py), each solved ONCE per process.

    K_ACC = 4e-3      the accuracy tests: every lane of law_reference.LANES is finite under both laws and both histories
    K_LOW = 1e-3      below the critical (b - a) / Dc on the stiff lanes: the step history's slip-law RK4 is non-finite on exactly
                      the lanes Dc = 5, 6, 8, in float64 and in long double alike
    K_WHY = 2e-3      the data of the target test: friction from Dc = 20, so k Dc = 0.04, not the coupling's 0.1
    DC64, K64         Dc = 64 with k = 1e-2 * 10 / 64: k Dc == 0.1 exactly, where the new kernels are the coupled ones bit for bit

The matrix entries are law_matrix_cases' `ab`, `undamped_ab`, `k1zero`, `sub2` and `chunks_ab`; the yardstick of an entry is formed
by law_matrix_cases' rule: the larger of the two CPU arrangements' largest error against long double, floored at the default
(coupled) model's.
"""
import functools

import numpy as np

import law_cases as C
import law_matrix_cases as M
import law_reference as R
import observe_cases as OC
import observe_reference as O
import stiff_reference as S

K_ACC, K_LOW, K_WHY = 4e-3, 1e-3, 2e-3
DC64 = 64.0
K64 = 1e-2 * 10 / 64
ENTRIES = ("ab", "undamped_ab", "k1zero", "sub2", "chunks_ab")
LOW_LANES = (5.0, 6.0, 8.0)  # the lanes K_LOW sends into stick-slip (step history, slip law)
WHY_NODES, WHY_SEED = 781, 7


def lanes70():
    """-> index into the twelve lanes of the 70: the twelve tiled, a full wave and a partial second one"""
    return np.arange(70) % len(R.LANES)


@functools.lru_cache(maxsize=None)
def solve(name, history, law, k=K_ACC):
    """law_matrix_cases.solve with the stiffness k: one entry (or "default": the default model, the model's (a, b)) under `history` and `law`, all four observables from one solve per
    solver -> dict(m, dc, a, b, vl, spec, lane, ext {observable: series}, err_spec, err_lane {observable: per-lane error}, own,
    yardstick {observable: .}).  Lanes whose long-double series is not finite carry a NaN error and are left out of own."""
    m, dc, a, b = (C.spec(), np.asarray(R.LANES), None, None) if name == "default" else M.config(name)
    vl = R.table(m, history)
    spec, lane = S.trajectory(m, k, dc, vl, law, a, b), S.trajectory_lane(m, k, dc, vl, law, a, b)
    ext = S.trajectory(m, k, dc, vl, law, a, b, dtype=R.LD)
    with np.errstate(all="ignore"):
        err_spec = {o: M.error(o, spec[o], ext[o]) for o in O.OBSERVABLES}
        err_lane = {o: M.error(o, lane[o], ext[o]) for o in O.OBSERVABLES}
    finite = np.isfinite(np.asarray(ext["velocity"], dtype=np.float64)).all(axis=0)
    own = {o: float(max(err_spec[o][finite].max(), err_lane[o][finite].max())) for o in O.OBSERVABLES}
    floor = dict(OC.precision_set(history, law)["yardstick"], acc=C.precision_set(history, law)["yardstick"])
    yardstick = {o: max(own[o], floor[o]) for o in O.OBSERVABLES}
    return {"m": m, "dc": dc, "a": a, "b": b, "vl": vl, "spec": spec, "lane": lane, "ext": ext, "err_spec": err_spec, "err_lane": err_lane,
            "finite": finite, "own": own, "yardstick": yardstick}


def coupled_lanes():
    """-> (dc, a, b): twelve lanes at Dc = 64 with law_matrix_cases.lane_ab's per-lane (a, b)"""
    a, b = M.lane_ab()
    return np.full(a.size, DC64), a, b


@functools.lru_cache(maxsize=None)
def why_problem(history):
    """The friction data set of the constant-k model: Dc = 20, (a, b) the defaults, k = K_WHY, nsteps 500 under `history`, noise 5 %
    of the excursion from default_rng(WHY_SEED); and the float64 specification's SSq of the constant-k and of the coupled model
    on WHY_NODES uniform nodes over BF_BOX -> dict(m, vl, data, x, ssq_stiff, ssq_coupled)"""
    m = C.spec()
    vl = R.table(m, history)
    clean = S.forward(m, K_WHY, [R.BF_TRUTH], vl, "aging", "mu")[0][:, 0]
    data = clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(WHY_SEED).standard_normal(clean.size)
    x = np.linspace(R.BF_BOX[0], R.BF_BOX[1], WHY_NODES)
    return {"m": m, "vl": vl, "data": data, "x": x, "ssq_stiff": S.forward(m, K_WHY, x, vl, "aging", "mu", data=data)[1],
            "ssq_coupled": O.forward(m, x, vl, "aging", "mu", data=data)[1]}
