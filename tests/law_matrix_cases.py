"""
What tests/test_observe_reference.py (CPU) and tests/test_gpu_law_matrix.py share (a test helper): the CONFIGURATION MATRIX of
the state-law solve beyond the default model — per-lane (a, b), no damping, k1 = 0, substeps > 1, a table staged in two
chunks, and models whose V_ref, mu_ref, mu_t_zero, k1 and t_start are not the defaults — each entry solved ONCE per process
under a history and a law by the two float64 arrangements and the long-double specification (tests/observe_reference.py), on
the twelve lanes of law_reference.LANES.

    name                 model                                                        per-lane (a, b)
    ab                   default                                                      yes
    undamped_ab          RadiationDamping = False                                     yes
    k1zero               k1 = 0                                                       no
    sub2                 nsteps 500, substeps 2 (the table resident in LDS)           no
    chunks_ab            nsteps 900, substeps 4 (the table in two chunks)             yes
    nondefault           nsteps 400, t_start 1.5, t_final 37, the attributes ND       no
    nondefault_sub3_ab   as nondefault, substeps 3                                    yes
    si                   V_ref = 1e-6, k1 / V_ref, the lanes LANES * 1e-6             no
    pow2                 V_ref = 2^-20, k1 / V_ref, the lanes LANES * 2^-20           no     (the exact-scaling tests only)

ND is the attribute set of tests/golden/forward_nondefault.json.  The per-lane (a, b) are default_rng(12)'s, a ~ U(0.009,
0.013) then b ~ U(0.012, 0.016).  `si` and `pow2` are the default problem in other units: the damping coefficient carries units
of 1 / velocity (k1 v / a is what the equations hold), so k1 is divided by V_ref along with Dc being multiplied by it, as
tests/test_gpu_parity.py's test_forward_is_scale_free_in_v_ref does; then theta and mu are the default model's and velocity and
acc are V_ref times it.

The yardstick of an entry is the larger of its two CPU arrangements' largest error against long double, FLOORED at the default
model's (observe_cases.precision_set / law_cases.precision_set): the device's rounding error does not shrink because the CPU's
happened to be small on twelve lanes (`nondefault`'s are 20 x below the default ones).
"""
import functools

import numpy as np

import law_cases as C
import law_reference as R
import observe_cases as OC
import observe_reference as O

ND = dict(V_ref=1.7, mu_ref=0.55, mu_t_zero=0.58, k1=3e-7, a=0.012, b=0.0155)  # tests/golden/forward_nondefault.json's attrs
HISTORIES = ("step", "hold")
POW2 = 2.0 ** -20


def _nondefault(substeps=1):
    m = R.Spec(400, 1.5, 37.0, substeps)
    for k, v in ND.items():
        setattr(m, k, v)
    return m


def _units(V_ref):
    m = C.spec()
    m.k1 = m.k1 / V_ref
    m.V_ref = V_ref
    return m


# name -> (the R.Spec, per-lane (a, b)?, the factor on R.LANES)
MATRIX = {
    "ab": (lambda: C.spec(), True, 1.0),
    "undamped_ab": (lambda: C.spec(RadiationDamping=False), True, 1.0),
    "k1zero": (lambda: C.spec(k1=0.0), False, 1.0),
    "sub2": (lambda: C.spec(500, 2), False, 1.0),
    "chunks_ab": (lambda: C.spec(900, 4), True, 1.0),
    "nondefault": (lambda: _nondefault(), False, 1.0),
    "nondefault_sub3_ab": (lambda: _nondefault(3), True, 1.0),
    "si": (lambda: _units(1.0e-6), False, 1.0e-6),
}
NAMES = tuple(MATRIX)
EXTRA = {"pow2": (lambda: _units(POW2), False, POW2)}  # not a row of the matrix: the exact-scaling test's model


def lane_ab():
    """the per-lane (a, b) of the entries that have them"""
    rng = np.random.default_rng(12)
    return rng.uniform(0.009, 0.013, len(R.LANES)), rng.uniform(0.012, 0.016, len(R.LANES))


def config(name):
    """-> (m, dc, a, b): the entry's R.Spec, its lanes and its per-lane (a, b) or (None, None)"""
    make, ab, factor = (MATRIX.get(name) or EXTRA[name])
    a, b = lane_ab() if ab else (None, None)
    return make(), np.asarray(R.LANES) * factor, a, b


def error(obs, series, ext):
    """per lane, the project's measure of a series against the long-double one: relative to max|acc| for the acceleration
    (R.rel_error), to the excursion otherwise (O.range_error)"""
    return R.rel_error(series, ext) if obs == "acc" else O.range_error(series, ext)


@functools.lru_cache(maxsize=None)
def solve(name, history, law):
    """One entry under `history` and `law`, all four observables from one solve per solver -> dict(m, dc, factor, a, b, vl, spec, lane
    (the two float64 arrangements), ext (long double): {observable: series}, err_spec, err_lane {observable: per-lane error},
    own {observable: the larger of the two arrangements' largest error}, yardstick {observable: own floored at the default
    model's})"""
    m, dc, a, b = config(name)
    vl = R.table(m, history)
    spec, lane = O.trajectory(m, dc, vl, law, a, b), O.trajectory_lane(m, dc, vl, law, a, b)
    ext = O.trajectory(m, dc, vl, law, a, b, dtype=R.LD)
    err_spec = {k: error(k, spec[k], ext[k]) for k in O.OBSERVABLES}
    err_lane = {k: error(k, lane[k], ext[k]) for k in O.OBSERVABLES}
    own = {k: float(max(err_spec[k].max(), err_lane[k].max())) for k in O.OBSERVABLES}
    floor = dict(OC.precision_set(history, law)["yardstick"], acc=C.precision_set(history, law)["yardstick"])
    yardstick = {k: max(own[k], floor[k]) for k in O.OBSERVABLES}
    return {"m": m, "dc": dc, "factor": (MATRIX.get(name) or EXTRA[name])[2], "a": a, "b": b, "vl": vl, "spec": spec, "lane": lane, "ext": ext, "err_spec": err_spec, "err_lane": err_lane,
            "own": own, "yardstick": yardstick}
