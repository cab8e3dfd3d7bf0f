"""
The adaptive proposal of adapt_mode = "am" in mcmc_kernel and mcmc_f32x2_kernel against its long-double specification
(tests/adapt_reference.py, which states the history, the boundaries, the bound and the procedure): the whole-history shifted sums,
rsf::window_covariance, the Cholesky factor the d = 3 kernels keep in LDS, and the window that store_window / load_window carry
between launches.  tests/test_adapt_reference.py runs the same procedure on the CPU checker.
"""
import pytest

import adapt_reference as ar

pytestmark = pytest.mark.gpu


def _engine(pkg, case):
    return pkg.Engine(mem="host", block_threads=case.get("block_threads", 0))


@pytest.mark.parametrize("name", sorted(ar.CASES))
def test_am_proposal(pkg, oracle_mod, name):
    case = ar.CASES[name]
    with _engine(pkg, case) as e:
        assert e.lib.rsf_backend() == b"hip-gfx950"
        res = ar.run_case(e, oracle_mod, case, label=f"GPU case {name}")
    print(f"GPU case {name}: {res}")
    assert res["v_ratio"] <= 1.0 and res["step_ratio"] <= 1.0


@pytest.mark.parametrize("name", ["b", "e"])
def test_am_set_state_keeps_the_history(pkg, oracle_mod, name):
    """set_state(V = V3) between two boundaries, d = 3 (float64 and float32): the factor in LDS is rebuilt from the new V at the next
    launch — the steps up to the next boundary are chol(V3) z — and the history is not reset: from the boundary on the steps are
    chol(V_k) z with V_k of the whole trace."""
    case = dict(ar.CASES[name], launches=(3, 9, 11))
    with _engine(pkg, case) as e:
        res = ar.run_case(e, oracle_mod, case, set_V3_after=0, label=f"GPU case {name} + set_state")
    print(f"GPU case {name} + set_state: {res}")
    assert res["v3_steps"] > 0
