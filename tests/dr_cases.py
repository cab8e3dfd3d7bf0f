"""
Cases the delayed-rejection sampler's CPU and GPU tests share (TEST INFRASTRUCTURE ONLY): the closed-form legs of the target
tests and the crafted rows of the split-path test.
"""
import numpy as np

import posterior_reference as R

_REF = {}


def closed_reference(d):
    if d not in _REF:
        _REF[d] = R.closed_reference(d)
    return _REF[d]


def rows_fn(fn, d):
    """fn(*columns) → ssq_fn(points (m, d))"""
    return lambda q: fn(*np.asarray(q, np.float64).reshape(-1, d).T)


# the legs of the target tests: (d, scale of the factor, gamma).  L = scale chol(V), V = K^-1 S0 / (2 shape - d), about the
# posterior's covariance (posterior_reference.run_injected's V).  At (3, 3, 0.3) about 65 % of the first proposals leave the box.
LEGS = ((1, 3.0, 0.3), (3, 1.0, 0.2), (3, 3.0, 0.3))
# the legs on which the two wrong rules (dr_reference's mutants) must fail check(): the wide d = 3 leg does not detect a dropped
# log q, so nothing is asserted of the mutants there
MUTANT_LEGS = ((1, 3.0, 0.3), (3, 1.0, 0.2))
C_TARGET = 262144  # at 65536 some mutants pass
CHECKPOINTS = (4, 8)
SEED = 31


def closed_factor(c, scale):
    d = len(c["q0"])
    V = np.linalg.inv(np.asarray(c["K"], np.float64)) * c["S0"] / (2 * c["shape"] - d)
    return scale * np.linalg.cholesky(V)


# ---- the split-path problem: 257 chains (a partial wave beyond a workgroup) and rows crafted for every way an iteration ends -----
SPLIT_N, SPLIT_ITERS, SPLIT_SEED, SPLIT_OFFSET, SPLIT_GAMMA = 257, 4, 17, 1000, 0.3
BAD_SSQ = (np.inf, np.nan, 0.0, -1.0)


def split_problem(d):
    """→ dict(lo, hi, L, shape, fn, q0 (n, d), bad_l {row: start l}, fix(stage, ssq) → ssq, rows {name: indices}).  The closed form of
    posterior_reference.CLOSED[3] in its first d parameters; behind SPLIT_N random chains:
        face     6 chains next to each face of the box (1e-7 of the width inside): about half of their first proposals leave
                 through it, and then about half of their second ones;
        bad1     4 chains whose stage-1 SSq is planted as inf, NaN, 0, -1 (l1 = -inf: on to stage 2, without A and B);
        bad2     4 chains whose stage-1 SSq is inf and whose stage-2 SSq is inf, NaN, 0, -1 (rejected);
        order    2 chains with a planted finite l1 (SSq 1e30) and l2 below it (SSq 1e40) or equal to it (1e30): rejected, l1 >= l2;
        low1     2 chains with the planted l1 (SSq 1e30) and their own l2: A and B at a large negative argument;
        stuck    3 chains: one outside the box, one with l = -inf, one with l = NaN."""
    c = R.CLOSED[3]
    lo, hi = np.array(c["lo"][:d]), np.array(c["hi"][:d])
    K, qc = np.asarray(c["K"])[:d, :d], np.asarray(c["q0"])[:d]
    fn = rows_fn(R.quadratic_ssq(c["S0"], qc, K), d)
    L = 0.5 * np.linalg.cholesky(np.linalg.inv(K) / (2 * c["shape"] - d))
    rng = np.random.default_rng(100 + d)
    mid, w = 0.5 * (lo + hi), hi - lo
    rows, q = {}, [rng.uniform(lo + 0.05 * w, hi - 0.05 * w, (SPLIT_N, d))]
    at = SPLIT_N

    def add(name, pts):
        nonlocal at
        pts = np.atleast_2d(pts)
        rows[name] = np.arange(at, at + len(pts))
        q.append(pts)
        at += len(pts)

    for p in range(d):
        for side, edge in (("lo", lo[p] + 1e-7 * w[p]), ("hi", hi[p] - 1e-7 * w[p])):
            pts = np.tile(mid, (6, 1))
            pts[:, p] = edge
            add(f"face {p} {side}", pts)
    add("bad1", np.tile(mid, (4, 1)))
    add("bad2", np.tile(mid, (4, 1)))
    add("order", np.tile(mid, (2, 1)))
    add("low1", np.tile(mid, (2, 1)))
    out = mid.copy()
    out[0] = hi[0] + 1.0
    add("stuck", np.stack([out, mid, mid]))
    bad_l = {int(rows["stuck"][1]): -np.inf, int(rows["stuck"][2]): np.nan}

    def fix(stage, ssq):
        ssq = ssq.copy()
        if stage == 1:
            ssq[rows["bad1"]] = BAD_SSQ
            ssq[rows["bad2"]] = np.inf
            ssq[rows["order"]] = 1e30
            ssq[rows["low1"]] = 1e30
        else:
            ssq[rows["bad2"]] = BAD_SSQ
            ssq[rows["order"]] = (1e40, 1e30)
        return ssq

    return dict(lo=lo, hi=hi, L=L, shape=c["shape"], fn=fn, q0=np.ascontiguousarray(np.concatenate(q)), bad_l=bad_l, fix=fix, rows=rows)


def split_coverage(d, steps, prob):
    """what the crafted rows must have met over the iterations (steps: dr_reference.step's dicts): → list of what is missing"""
    rows, lo, hi = prob["rows"], prob["lo"], prob["hi"]
    missing = []
    for p in range(d):
        for side in ("lo", "hi"):
            r = rows[f"face {p} {side}"]
            edge = (lambda y: y[r, p] <= lo[p]) if side == "lo" else (lambda y: y[r, p] >= hi[p])
            if not any((~st["stuck"][r] & edge(st["y1"])).any() for st in steps):
                missing.append(f"y1 through face {p} {side}")
            if not any((st["pending"][r] & ~st["in2"][r] & edge(st["y2"])).any() for st in steps):
                missing.append(f"y2 through face {p} {side}")
    for st in steps:
        for name in ("bad1", "bad2", "order", "low1"):
            r = rows[name]
            if not (st["in1"][r].all() and not st["acc1"][r].any() and st["pending"][r].all() and st["in2"][r].all()):
                missing.append(f"{name}: a row left the box or was accepted at stage 1")
        if st["acc2"][rows["bad2"]].any() or st["acc2"][rows["order"]].any():
            missing.append("a bad SSq2 or an l1 >= l2 was accepted")
        if not (np.isneginf(st["l1"][rows["bad1"]]).all() and np.isfinite(st["l1"][rows["order"]]).all() and st["rejected2"][rows["order"]].all()):
            missing.append("bad1 / order: l1 is not what was planted")
        if not st["stuck"][rows["stuck"]].all() or st["stuck"].sum() != 3:
            missing.append("the stuck rows")
    if not any(st["acc2"][rows["bad1"]].any() for st in steps) or not any(st["acc2"][rows["low1"]].any() for st in steps):
        missing.append("no stage-2 acceptance after a bad SSq1 / after the planted l1")
    return missing
