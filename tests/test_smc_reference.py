"""
CPU tests of tests/smc_reference.py, the specification of include/rsf_smc.h: they make the specification trustworthy (its log I
is unbiased on the ratio scale and its final particles are the target, against the quadrature truths of
tests/posterior_reference.py and tests/evidence_cases.CLOSED_TRUTH) and measure the constants of tests/smc_cases.py.
"""
import numpy as np
import pytest

import evidence_cases
import posterior_reference as R
import smc_cases as cases
import smc_reference as ref

LD = np.longdouble


def test_philox_known_answers():
    # Random123's known-answer vectors for philox4x32-10
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        assert tuple(int(x) for x in ref.philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]) == want


@pytest.mark.parametrize("d", [1, 3])
def test_exact_integral_and_final_sample(d):
    post, fn, c = R.closed_reference(d)
    ssq_fn = lambda q: fn(*np.asarray(q).reshape(-1, d).T)
    truth = evidence_cases.CLOSED_TRUTH[d]
    runs = [ref.run(ssq_fn, c["lo"], c["hi"], cases.N_SPEC, c["shape"], seed=s) for s in range(cases.R_SPEC)]
    logi = np.array([r["log_integral"] for r in runs])
    ratio = np.exp(logi - truth)
    z = (ratio.mean() - 1.0) / (ratio.std(ddof=1) / np.sqrt(ratio.size))
    print(f"d = {d}: mean of exp(log I - truth) {ratio.mean():.5f}, z {z:+.2f}, sd of log I {logi.std(ddof=1):.4f} (SPEC_SD {cases.SPEC_SD[d]}), "
          f"{np.mean([len(r['stages']) for r in runs]):.1f} stages, accept rate {np.mean([s['accept_rate'] for r in runs for s in r['stages']]):.3f}")
    assert abs(z) < R.Z_MAX
    # the recorded constant is this measurement: the same seeds give the same number
    assert logi.std(ddof=1) == pytest.approx(cases.SPEC_SD[d], rel=0.02)
    # the final particles: mean and variance per parameter, the standard error from the replicates
    names = ("Dc",) if d == 1 else ("Dc", "a", "b")
    for p, name in enumerate(names):
        mg = post.marg[name]
        m, v = np.array([r["q"][:, p].mean() for r in runs]), np.array([r["q"][:, p].var() for r in runs])
        zm = (m.mean() - mg.mean) / (m.std(ddof=1) / np.sqrt(m.size))
        zv = (v.mean() - mg.var) / (v.std(ddof=1) / np.sqrt(v.size))
        print(f"d = {d} {name}: mean z {zm:+.2f}, variance z {zv:+.2f}")
        assert abs(zm) < R.Z_MAX and abs(zv) < R.Z_MAX
    for r in runs:
        assert r["stages"][-1]["beta"] == 1.0 and ref.inbox(r["q"], c["lo"], c["hi"]).all() and np.isfinite(r["l"]).all()


@pytest.mark.parametrize("n", [1, 5, 1037, 16421])
def test_systematic_resampling_counts(n):
    l = cases.exact_l(n)
    for u in (2.0 ** -53, 0.37, 1.0):
        for dtype in (LD, np.float64):
            cum, anc = ref.resample(l, 0.25, 0.0, u, dtype)
            np.testing.assert_array_equal(np.asarray(cum, dtype=np.float64), np.cumsum(np.isfinite(l)))  # exact prefix sums
            counts = np.bincount(anc, minlength=n)
            w = np.isfinite(l).astype(np.float64)
            want = n * w / w.sum()
            assert ((counts == np.floor(want)) | (counts == np.ceil(want))).all() and counts.sum() == n
            assert (np.diff(anc) >= 0).all() and (counts[~np.isfinite(l)] == 0).all()


def test_float64_distance_sizes_the_bounds():
    e_init = e_sums = e_cum = 0.0
    for d, (lo, hi) in cases.BOXES.items():
        a, b = ref.init(11, cases.OFFSET, 1037, lo, hi, LD), ref.init(11, cases.OFFSET, 1037, lo, hi, np.float64)
        e_init = max(e_init, float(np.abs((a - b) / a).max()))
        assert ref.inbox(a, lo, hi).all() and ref.inbox(b, lo, hi).all()
    mism = 0
    for n in cases.DIST_NS:
        l = cases.crafted_l(n)
        h64, hld = ref.weight_sums(l, cases.DELTAS, None, np.float64), ref.weight_sums(l, cases.DELTAS, None, LD)
        assert h64[:3] == hld[:3] and h64[1] + h64[2] == n
        e_sums = max(e_sums, float(np.abs((h64[3].astype(LD) - hld[3]) / hld[3]).max()))
        for delta in cases.DELTAS[1:]:
            c64, a64 = ref.resample(l, delta, h64[0], 0.37, np.float64)
            cld, ald = ref.resample(l, delta, h64[0], 0.37, LD)
            nz = cld > cases.CUM_FLOOR
            e_cum = max(e_cum, float(np.abs((c64[nz].astype(LD) - cld[nz]) / cld[nz]).max()) if nz.any() else 0.0)
            mism = max(mism, int((a64 != ald).sum()) / n)
    print(f"float64 against long double: init {e_init:.3e} (relative), sums {e_sums:.3e} (relative), cum {e_cum:.3e} (relative); "
          f"largest fraction of differing ancestors {mism:.2e}")
    assert e_init <= cases.DIST_INIT and e_sums <= cases.DIST_SUMS and e_cum <= cases.DIST_CUM
    assert e_sums >= cases.DIST_SUMS / 4 and e_cum >= cases.DIST_CUM / 4  # the recorded distances are these measurements, not slack
    assert mism <= 1e-3


@pytest.mark.parametrize("d", [1, 3])
def test_float64_run_follows_the_long_double_run(d):
    """The chain test of tests/test_gpu_smc.py allows an ancestor to differ only next to a boundary of cum, at most 0.1 % of n: the
    specification in plain float64 against long double stays under that cap on the same inputs."""
    _, fn, c = R.closed_reference(d)
    ssq_fn = lambda q: fn(*np.asarray(q).reshape(-1, d).T)
    a = ref.run(ssq_fn, c["lo"], c["hi"], 1037, c["shape"], seed=3, history=True)
    b = ref.run(ssq_fn, c["lo"], c["hi"], 1037, c["shape"], seed=3, dtype=np.float64, history=True)
    assert [s["beta"] for s in a["stages"]] == [s["beta"] for s in b["stages"]]
    diff = sum(int((x["ancestors"] != y["ancestors"]).sum()) for x, y in zip(a["history"], b["history"]))
    print(f"d = {d}: {len(a['stages'])} stages, {diff} differing ancestors")
    assert diff <= 1e-3 * 1037
    if diff == 0:
        width = np.asarray(c["hi"]) - np.asarray(c["lo"])
        assert float((np.abs(a["q"] - b["q"]) / width).max()) <= cases.TOL_CHAIN
        assert float(np.abs(a["l"] - b["l"]).max()) <= cases.TOL_CHAIN * c["shape"]


def test_choose_delta_and_refusals():
    l = cases.crafted_l(1037)
    fn = lambda cand: ref.weight_sums(l, cand, None, LD)
    delta, lmax, sw, ess, beta = ref.choose_delta(0.0, 0.5, fn)
    nfin = int(np.isfinite(l).sum())
    assert 0.0 < delta < 1.0 and beta == delta and ess >= 0.5 * nfin
    # the step is the largest on the search's grid: a step one resolution further fails
    _, _, _, s2 = ref.weight_sums(l, [delta * (1 + 16.0 ** (1 - ref.ROUNDS)) + 16.0 ** -ref.ROUNDS], None, LD)
    assert float(s2[0][0] ** 2 / s2[0][1]) < 0.5 * nfin
    # equal weights: one stage to beta = 1
    assert ref.choose_delta(0.25, 0.5, lambda cand: ref.weight_sums(np.zeros(63), cand, None, LD))[4] == 1.0
    with pytest.raises(ValueError, match="-inf"):
        ref.weight_sums(np.full(5, -np.inf), [0.5])
    with pytest.raises(ValueError):
        ref.weight_sums(np.array([0.0, np.nan]), [0.5])
