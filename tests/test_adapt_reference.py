"""
The adaptive proposal of adapt_mode = "am" on the CPU checker, against its long-double specification (tests/adapt_reference.py):
the covariance a chain holds after every launch is that of its own trace up to the last boundary, the steps it takes are the
factor of the window in force times the iteration's normals — across launches, after set_state(V=), for both chains of a float32
lane, and frozen under adapt_mode none.  tests/test_gpu_adapt.py runs the same procedure on the GPU.
"""
import numpy as np
import pytest

import adapt_reference as ar


def _engine(pkg, oracle_lib, case):
    return pkg.Engine(lib=oracle_lib, block_threads=case.get("block_threads", 0))


@pytest.mark.parametrize("name", sorted(ar.CASES))
def test_am_proposal_on_the_checker(pkg, oracle_lib, oracle_mod, name):
    case = ar.CASES[name]
    with _engine(pkg, oracle_lib, case) as e:
        res = ar.run_case(e, oracle_mod, case, label=f"checker case {name}")
    print(f"checker case {name}: {res}")
    assert res["v_ratio"] <= 1.0 and res["step_ratio"] <= 1.0


@pytest.mark.parametrize("name", ["b", "e"])
def test_am_set_state_keeps_the_history_on_the_checker(pkg, oracle_lib, oracle_mod, name):
    """set_state(V = V3) between two boundaries, d = 3: the steps up to the next boundary are chol(V3) z, from the boundary on
    chol(V_k) z with V_k of the whole history, the iterations before set_state included."""
    case = dict(ar.CASES[name], launches=(3, 9, 11))
    with _engine(pkg, oracle_lib, case) as e:
        res = ar.run_case(e, oracle_mod, case, set_V3_after=0, label=f"checker case {name} + set_state")
    print(f"checker case {name} + set_state: {res}")
    assert res["v3_steps"] > 0


def test_reference_windows_are_numpys_covariance():
    """the long-double windows against np.cov / np.linalg.cholesky on a random trace, and kappa on a constructed one"""
    rng = np.random.default_rng(5)
    N, C, d, I = 23, 9, 3, 7
    scale = np.array([30.0, 2e-4, 3e-4])
    tq = np.array([1000.0, 0.011, 0.014]) + np.cumsum(rng.standard_normal((N, C, d)) * scale, axis=0)
    q0 = tq[0] - scale
    win = ar.windows(tq, q0, ar.BOX_LO, ar.BOX_HI, I)
    assert sorted(win) == [7, 14, 21]
    eps = (1e-6 * (np.array(ar.BOX_HI) - np.array(ar.BOX_LO))) ** 2
    for k, w in win.items():
        for c in range(C):
            V = 2.38 ** 2 / d * (np.cov(tq[:k, c].T) + np.diag(eps))
            np.testing.assert_allclose(w["V"][c].astype(np.float64), V, rtol=1e-9, atol=0)
            np.testing.assert_allclose(w["L"][c].astype(np.float64), np.linalg.cholesky(V), rtol=1e-7)
            kappa = ((tq[:k, c].mean(axis=0) - q0[c]) ** 2 / tq[:k, c].var(axis=0, ddof=1)).max()
            np.testing.assert_allclose(w["kappa"][c], kappa, rtol=1e-9)
    # a chain that never moves: kappa 0, V = (2.38^2 / d) diag(eps); one that moved once, at the start: the shift over eps
    still = np.tile(q0[None, :1], (I, 1, 1))
    w = ar.windows(still, q0[:1], ar.BOX_LO, ar.BOX_HI, I)[I]
    assert w["kappa"][0] == 0.0
    np.testing.assert_allclose(w["V"][0].astype(np.float64), 2.38 ** 2 / d * np.diag(eps), rtol=1e-15)
    w = ar.windows(still + np.array([3.0, 0.0, 0.0]), q0[:1], ar.BOX_LO, ar.BOX_HI, I)[I]
    np.testing.assert_allclose(w["kappa"][0], 9.0 / eps[0], rtol=1e-12)
