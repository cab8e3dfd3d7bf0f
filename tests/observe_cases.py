"""
What tests/test_observe_reference.py (CPU) and tests/test_gpu_observe.py share (a test helper): the precision lane sets with
both float64 arrangements and the long-double specification solved ONCE per process (tests/observe_reference.py), and the
Bayes-factor problem on friction data.
"""
import functools

import numpy as np

import law_cases as C
import law_reference as R
import observe_reference as O

GATED = ("mu", "theta", "velocity")  # the observables tested against long double here; "acc" is tests/test_gpu_law.py's


@functools.lru_cache(maxsize=None)
def precision_set(history, law):
    """R.LANES at nsteps 500, substeps 1 under `history` and `law`, all four observables from one solve per arrangement →
    dict(m, dc, vl, spec, lane (the two float64 arrangements), ext (long double): {observable: series}, err_spec, err_lane
    {observable: per-lane range_error}, yardstick {observable: the larger of the two arrangements' largest range_error})"""
    m = C.spec()
    dc = np.asarray(R.LANES)
    vl = R.table(m, history)
    spec, lane, ext = O.trajectory(m, dc, vl, law), O.trajectory_lane(m, dc, vl, law), O.trajectory(m, dc, vl, law, dtype=R.LD)
    err_spec = {k: O.range_error(spec[k], ext[k]) for k in O.OBSERVABLES}
    err_lane = {k: O.range_error(lane[k], ext[k]) for k in O.OBSERVABLES}
    yardstick = {k: float(max(err_spec[k].max(), err_lane[k].max())) for k in O.OBSERVABLES}
    return {"m": m, "dc": dc, "vl": vl, "spec": spec, "lane": lane, "ext": ext, "err_spec": err_spec, "err_lane": err_lane, "yardstick": yardstick}


@functools.lru_cache(maxsize=None)
def friction_problem(truth):
    """The step-history FRICTION data set whose truth is `truth` (Dc = 20, noise 5 % of max|mu - mu_0|) with the float64
    specification's posteriors on 4001 uniform trapezoid nodes over [5, 200] → dict(m, vl, data, log_evidence, mean, sd
    {law: .}, ssq {law: .}, log_bayes_factor = slip - ageing)"""
    m = C.spec()
    vl = R.table(m, "step")
    data = O.bf_data(m, vl, truth, "mu")
    post, ssq = O.bf_posteriors(m, vl, data, "mu")
    ev = {law: post[law][0] for law in R.LAWS}
    return {"m": m, "vl": vl, "data": data, "log_evidence": ev, "mean": {law: post[law][1] for law in R.LAWS}, "sd": {law: post[law][2] for law in R.LAWS},
            "ssq": ssq, "log_bayes_factor": ev["slip"] - ev["aging"]}


@functools.lru_cache(maxsize=None)
def acc_sd(truth):
    """posterior SD of Dc under the TRUE law of law_cases.bayes_factor_problem(truth): the same problem on acceleration data"""
    p = C.bayes_factor_problem(truth)
    x = np.linspace(R.BF_BOX[0], R.BF_BOX[1], R.BF_NODES)
    w = R.trapezoid_weights(x)
    l = -R.LD(0.5 * R.nout(p["m"])) * np.log(np.asarray(p["ssq"][truth], dtype=R.LD))
    pr = w * np.exp(l - l.max())
    pr = pr / pr.sum()
    mean = float((pr * x).sum())
    return float(np.sqrt((pr * (x - mean) ** 2).sum()))
