"""
CPU tests of the host side of the batched SMC populations (Engine.smc_batch): the replicates' summary against a long double
log-mean-exp, the enumeration of the populations (groups x replicates → data row, seed, offset) and the argument errors that are
raised before any device call.
"""
import numpy as np
import pytest

LD = np.longdouble


def test_summary_against_long_double(pkg):
    rng = np.random.default_rng(3)
    # log evidences far from 0 (exp overflows in float64 without the shift) and a group label that is not 0..G-1
    le = np.concatenate([3172.0 + 0.3 * rng.standard_normal(8), -4100.0 + 2.0 * rng.standard_normal(5), [12.5]])
    group = np.array([7] * 8 + [2] * 5 + [9])
    got = pkg.smc_batch_summary(le, group)
    assert [g["group"] for g in got] == [7, 2, 9] and [g["replicates"] for g in got] == [8, 5, 1]
    for g in got[:2]:
        x = le[group == g["group"]].astype(LD)
        top = x.max()
        z = np.exp(x - top)
        want = top + np.log(z.mean())
        rel = z / z.mean()
        se = np.sqrt(((rel - rel.mean()) ** 2).sum() / (x.size - 1)) / np.sqrt(LD(x.size))
        sd = np.sqrt(((x - x.mean()) ** 2).sum() / (x.size - 1))
        # a shifted sum of R terms in (0, 1] and one logarithm: a few ulp of the result
        assert abs(LD(g["log_evidence_mean"]) - want) <= 8 * np.spacing(abs(float(want)))
        assert g["log_evidence_sd"] == pytest.approx(float(sd), rel=1e-12) and g["log_evidence_se"] == pytest.approx(float(se), rel=1e-12)
        # Jensen: the logarithm of the mean evidence is not below the mean of the logarithms
        assert g["log_evidence_mean"] >= float(x.mean())
    one = got[2]
    assert one["log_evidence_mean"] == 12.5 and np.isnan(one["log_evidence_sd"]) and np.isnan(one["log_evidence_se"])
    # equal replicates: the mean is the value, no spread
    same = pkg.smc_batch_summary([5.0, 5.0, 5.0], [0, 0, 0])[0]
    assert same["log_evidence_mean"] == 5.0 and same["log_evidence_sd"] == 0.0 and same["log_evidence_se"] == 0.0
    with pytest.raises(ValueError):
        pkg.smc_batch_summary([1.0, 2.0], [0])
    with pytest.raises(ValueError):
        pkg.smc_batch_summary([], [])


def test_population_enumeration(pkg):
    pops = pkg.smc_batch_populations(3, replicates=2)
    np.testing.assert_array_equal(pops["group"], [0, 0, 1, 1, 2, 2])
    np.testing.assert_array_equal(pops["replicate"], [0, 1, 0, 1, 0, 1])
    np.testing.assert_array_equal(pops["seed"], [0, 1, 0, 1, 0, 1])  # what a loop over Engine.smc(seed=r) uses
    np.testing.assert_array_equal(pops["offset"], 0)
    assert (pops["group"].dtype, pops["seed"].dtype, pops["offset"].dtype) == (np.int32, np.uint64, np.int64)
    pops = pkg.smc_batch_populations(5, groups=[4, 1], seeds=100, offsets=7, replicates=3)
    np.testing.assert_array_equal(pops["group"], [4, 4, 4, 1, 1, 1])
    np.testing.assert_array_equal(pops["seed"], [100, 101, 102] * 2)
    np.testing.assert_array_equal(pops["offset"], 7)
    pops = pkg.smc_batch_populations(1, seeds=[9, 3], offsets=[0, 4096], replicates=2)
    np.testing.assert_array_equal(pops["seed"], [9, 3])
    np.testing.assert_array_equal(pops["offset"], [0, 4096])
    assert pkg.smc_batch_populations(8, replicates=8)["group"].size == pkg._abi.SMC_BATCH_MAX
    for bad in (dict(n_groups=0), dict(n_groups=2, replicates=0), dict(n_groups=2, groups=[2]), dict(n_groups=2, groups=[-1]),
                dict(n_groups=2, groups=[]), dict(n_groups=2, groups=[0.5]), dict(n_groups=2, seeds=[1, 2, 3], replicates=2),
                dict(n_groups=2, offsets=[1], replicates=2), dict(n_groups=2, seeds=-1), dict(n_groups=2, offsets=-5),
                dict(n_groups=13, replicates=5)):  # 65 populations
        with pytest.raises(ValueError):
            pkg.smc_batch_populations(**bad)


def test_argument_errors_before_any_device_call(pkg, cpu_engine):
    """On the checker engine, whose library has no rsf_smc_batch_* at all: each of these is refused in Python."""
    eng = cpu_engine
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.smc_batch(np.zeros(50), [0.0], [1.0], 10)
    model = pkg.RateStateModel(number_time_steps=50)
    eng.set_model(model, 1)
    data = np.zeros((2, eng.nout))
    for kw in (dict(lo=[0.0, 0.0], hi=[1.0, 1.0]),          # d = 2
               dict(ess_fraction=1.0), dict(steps=0), dict(steps=65), dict(max_stages=0),
               dict(groups=[2]), dict(replicates=33),       # a row that is not there; 66 populations
               dict(seeds=[1, 2])):                         # two seeds, one replicate
        args = dict(data=data, lo=[0.0], hi=[1.0e4], n=10)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.smc_batch(**args)
    with pytest.raises(ValueError, match="nout"):
        eng.smc_batch(np.zeros((2, eng.nout + 1)), [0.0], [1.0e4], 10)
    with pytest.raises(ValueError, match="nout"):
        eng.smc_batch(np.zeros((2, 2, eng.nout)), [0.0], [1.0e4], 10)
    q, l = np.zeros((3, 10, 1)), np.zeros((3, 10))
    with pytest.raises(ValueError, match=r"\(P, n, d\)"):
        eng.smc_batch_resample(np.zeros(10), l, 0.5, 0.0, 0.5)
    with pytest.raises(ValueError, match="populations"):
        eng.smc_batch_resample(q, np.zeros((2, 10)), 0.5, 0.0, 0.5)
    with pytest.raises(ValueError, match="one entry for each of the 3 populations"):
        eng.smc_batch_resample(q, l, [0.5, 0.5], 0.0, 0.5)
    with pytest.raises(ValueError, match="chol"):
        eng.smc_batch_move(q, l, data, 0, [0.0], [1.0e4], np.eye(1), 0.5, [1, 2, 3])
    with pytest.raises(ValueError, match="group"):
        eng.smc_batch_move(q, l, data, [0, 1], [0.0], [1.0e4], np.ones((3, 1, 1)), 0.5, [1, 2, 3])
    with pytest.raises(ValueError, match="steps"):
        eng.smc_batch_weight_sums(l, np.zeros((3, 17)))
    with pytest.raises(ValueError, match="steps"):
        eng.smc_batch_weight_sums(l, np.zeros((2, 4)))
    with pytest.raises(ValueError):
        eng.smc_batch_weight_sums(np.zeros(10), [0.5])
