"""
CPU tests of the extended-precision init reference (tests/init_extended.py) and of the float64 CPU restatement's init against it.

The helper's formula is pinned to the restatement's (oracle/rsf_oracle.c rsf_mcmc_init) by feeding it the restatement's own
float64 trajectories: the two must then agree to float64 rounding, observation groups included.  Fed the extended RK4 solves,
its distance from the restatement is the restatement's own init error — the yardstick the GPU tests hold init_kernel to
(tests/test_gpu_rk4_extended.py) — measured here on a handful of rk4_extended.CASES and pinned by caps.
"""
import numpy as np
import pytest

import init_extended as I
import rk4_extended as X

# The C restatement's init against the extended init, over every set of rk4_extended.CASES (fd 1e-6 for d = 1, 1e-4 for d = 3,
# prior_len 3, box (0, 0.005, 0.005) .. (100 max Dc, 0.02, 0.03)).  Measured max over every case: ssq0 and std2_0 1.6e-13
# (n2000_S1 narrow, d = 1); V 4.2e-7 for d = 1 (relative; n4000_S1_mu+5e-4 tight) and 8.7e-8 for d = 3 (every entry over
# sqrt(V_pp V_rr); n4000_S1_mu+5e-4 tight_edge).  On the cases below: 1.6e-13, 2.7e-7 (n2000_S1 narrow) and 3.2e-8
# (n500_S1_mu+5e-4 tight_edge); the caps leave 3.1x, 3.7x and 3.1x.  The trajectories' ~1e-13 rounding is amplified by
# 1 / fd times the relative sensitivity in V: well under the parity tests' 1e-9 (SSq), 2e-6 (d = 1 V) and 1e-4 (d = 3 V).
ORACLE_SSQ_CAP = 5e-13
ORACLE_V_CAP = {1: 1e-6, 3: 1e-7}
CPU_CASES = ["n500_S1", "nondefault", "n2000_S1", "n500_S1_mu+5e-4"]
FD = {1: 1e-6, 3: 1e-4}


def _inputs(p, d):
    q0 = p.dc.reshape(-1, 1) if d == 1 else np.stack([p.dc, p.a, p.b], axis=1)
    return q0, [0.0, 0.005, 0.005][:d], [100.0 * p.dc.max(), 0.02, 0.03][:d]


def test_cofactor_inverse_matches_numpy():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((200, 3, 3))
    S = A @ A.transpose(0, 2, 1) + 0.1 * np.eye(3)  # symmetric positive definite, as M is
    for M in (A, S):
        Mi = I.inverse3(M)
        np.testing.assert_allclose(Mi, np.linalg.inv(M), rtol=1e-9, atol=1e-12 * np.abs(Mi).max())
        np.testing.assert_allclose(Mi @ M, np.broadcast_to(np.eye(3), M.shape), atol=1e-10)
    L = I.inverse3(S.astype(np.longdouble))
    assert L.dtype == np.longdouble
    err = np.abs((L @ S.astype(np.longdouble)) - np.eye(3, dtype=np.longdouble)).max()
    assert err < 1e-14, err  # computed in extended precision (float64 would leave ~1e-14 .. 1e-13 at these condition numbers)


@pytest.mark.parametrize("d", [1, 3])
def test_helper_reproduces_the_restatement_from_its_own_trajectories(cpu_engine, oracle_mod, d):
    """The helper on the restatement's float64 solves (two observation groups): the restatement's ssq0, std2_0 and V to
    float64 rounding — the same perturbed points, denominators, degrees of freedom, prior box and group series."""
    p = X.Problem(oracle_mod.ModelSpec, "n500_S1")
    cpu_engine.set_model(p.m, p.m.substeps)

    def solve(m, dc, a, b):
        return (np.asarray(cpu_engine.forward(dc, a=a, b=b, want_acc=True)[1]),)

    q0, lo, hi = _inputs(p, d)
    acc, _ = X.forward_ext(p.m, p.dc[p.lanes("wide")][:1])
    data = np.stack([p.data, acc[:, 0].astype(np.float64) * 1.01])
    cpu_engine.mcmc_init(q0, data, lo, hi, prior_len=3, fd_rel_step=FD[d])
    _, ssq, std2, V = [np.asarray(x) for x in cpu_engine.get_state()]
    rs, r2, rV = I.initial_state_ext(solve, p.m, q0, data, FD[d], 3, lo, hi)
    assert I.rel(ssq, rs).max() < 1e-14 and I.rel(std2, r2).max() < 1e-14
    # d = 3: the restatement's own float64 Gram matrix and 3x3 inverse along the (Dc, a) ridge (measured 4.7e-10); a formula
    # slip — the unperturbed value in the denominator (1e-4), the degrees of freedom (0.6 %), the prior term — is >= 1e-4
    assert I.v_errors(V, rV).max() < (1e-13 if d == 1 else 2e-9), I.v_errors(V, rV).max()
    # the groups are really told apart: group 1's chains against group 0's series are far off
    rs0 = I.initial_state_ext(solve, p.m, q0, p.data, FD[d], 3, lo, hi)[0]
    half = q0.shape[0] // 2
    assert I.rel(ssq[half:], rs0[half:]).min() > 1e-3


@pytest.mark.parametrize("name", CPU_CASES)
def test_c_restatement_init_is_within_float64_rounding_of_the_reference(cpu_engine, oracle_mod, name):
    """rsf_mcmc_init of the float64 CPU restatement against the extended init, set by set, d = 1 and 3."""
    p = X.Problem(oracle_mod.ModelSpec, name)
    cpu_engine.set_model(p.m, p.m.substeps)
    worst = []
    for d in (1, 3):
        q0, lo, hi = _inputs(p, d)
        cpu_engine.mcmc_init(q0, p.data, lo, hi, prior_len=3, fd_rel_step=FD[d])
        _, ssq, std2, V = cpu_engine.get_state()
        rs, r2, rV = I.initial_state_ext(X.forward_ext, p.m, q0, p.data, FD[d], 3, lo, hi,
                                         acc0=p.ext["plain" if d == 1 else "ab"][0])
        es, e2, eV = I.rel(ssq, rs), I.rel(std2, r2), I.v_errors(V, rV)
        for s in p.sets:
            sl = p.lanes(s)
            print(f"{name:16s} d={d} {s:10s} ssq0 max {es[sl].max():.1e} med {np.median(es[sl]):.1e}  std2_0 max "
                  f"{e2[sl].max():.1e}  V max {eV[sl].max():.1e} med {np.median(eV[sl]):.1e}")
            worst.append((max(es[sl].max(), e2[sl].max()), eV[sl].max() / ORACLE_V_CAP[d], d, s))
    t = max(worst)
    assert t[0] < ORACLE_SSQ_CAP, t
    t = max(worst, key=lambda w: w[1])
    assert t[1] < 1, t
