"""
GPU tests of the joint posterior of the pooled draws (include/rsf_joint.h: rsf_pool_joint_partials / _finish, rsf_pool_kde2d,
rsf_pool_histogram2d, rsf_pool_hpd_levels; Engine.pool_joint*, pool_kde2d, pool_histogram2d, pool_hpd_levels;
PosteriorPool.joint and .corner) against the specification tests/joint_reference.py.  tests/joint_cases.py holds the inputs, the
bounds and the condition the moment bounds rest on.

Point sets of the 2-D KDE: m = 1, 63 (a 9 x 7 mesh over +-8 sd: exponents run past underflow), 1031, and — chosen after the
kernel's geometry was fixed at 256 threads x 4 points — 1025, one workgroup's chunk plus 1.

Measured on an MI355X (profiles/joint/gpu_joint_tests.log):
    moments, d in {1, 2, 3, 8}, n in {3, 5, 1037, 16421}, both centres, synthetic and real draws, shards, non-finite rows:
        mean error at most 0.075 of its bound; covariance error at most 4.5e-15 sqrt(c_pp c_qq) (bound 1e-11)
    kde2d, every point set, pair and block above: largest relative error 4.4e-12 where the reference exceeds 1e-290 (bound 1e-9),
        largest absolute error 2.1e-304 elsewhere (bound 1e-300); three uneven shards against one call 3.6e-14 (bound 1e-12)
    histogram2d: equal to the reference cell by cell.  57 tests in 5.9 s.
"""
import numpy as np
import pytest

import joint_cases as cases
import joint_reference as ref
import psis_cases

pytestmark = pytest.mark.gpu

CHUNK = 256 * 4  # points of one workgroup of pool_kde2d_kernel: kMaxBlock * kKde2dPoints
_MEMO = {}


def _real(pkg, oracle_lib, n):
    """psis_cases.real_draws at d = 3: computed once per size, shared, not changed."""
    if ("real", n) not in _MEMO:
        with pkg.Engine(lib=oracle_lib) as cpu:
            q = psis_cases.real_draws(pkg, cpu, n, 3, 400 + 3 + n)[1]
        q.setflags(write=False)
        _MEMO["real", n] = q
    return _MEMO["real", n]


def _block(pkg, oracle_lib, kind, n, d=3):
    if kind == "real":
        return _real(pkg, oracle_lib, n)
    if (kind, n, d) not in _MEMO:
        x = cases.synthetic(n, d)
        x.setflags(write=False)
        _MEMO[kind, n, d] = x
    return _MEMO[kind, n, d]


def _kde_ref(key, x2, pts, **kw):
    """The long-double reference of one (block, pair, point set): computed once, shared among the tests that need it."""
    if key not in _MEMO:
        r = ref.kde2d(x2, pts, **kw)
        r.setflags(write=False)
        _MEMO[key] = r
    return _MEMO[key]


@pytest.fixture(scope="module")
def dev_engine(pkg):
    e = pkg.Engine(mem="device")
    yield e
    e.close()


# ---- moments ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_moments(gpu_engine, dev_engine, d, n):
    x = cases.synthetic(n, d)
    for center in (None, cases.given_center(x)):
        c = x[0] if center is None else center
        cases.check_center(x, c)
        want = ref.moments(x, c)
        got = gpu_engine.pool_joint(x, center)
        assert got["n"] == n and got["nonfinite"] == 0 and got["cov"].shape == (d, d) and got["mean"].shape == (d,)
        cases.check_moments(got, want, f"moments d={d} n={n} centre {'first row' if center is None else 'given'}")
        assert np.array_equal(got["cov"], got["cov"].T) and np.all(np.diag(got["corr"]) == 1.0)
        part = gpu_engine.pool_joint_partials(x, center)
        assert part.shape == (ref.n_partials(d),)
        # device memory: the same kernels on the caller's own buffer, the same bits; and again
        import torch

        xd = torch.as_tensor(x, device="cuda")
        assert np.array_equal(dev_engine.pool_joint_partials(xd, center), part)
        assert np.array_equal(gpu_engine.pool_joint_partials(x, center), part)


@pytest.mark.parametrize("n", cases.SIZES_CAPPED)
@pytest.mark.parametrize("d", [3, 8])
def test_moments_past_the_grid_cap(gpu_engine, dev_engine, d, n):
    """The second and third trip of the grid-stride loop, in the unrolled (d = 3) and the run-time (d = 8) instantiation."""
    import torch

    x = _block(None, None, "synthetic", n, d)
    cases.check_center(x, x[0])
    got = gpu_engine.pool_joint(x)
    assert got["n"] == n and got["nonfinite"] == 0
    cases.check_moments(got, ref.moments(x, x[0]), f"moments d={d} n={n} (capped grid) centre first row")
    part = gpu_engine.pool_joint_partials(x)
    assert np.array_equal(dev_engine.pool_joint_partials(torch.tensor(x, device="cuda")), part)


def test_moments_of_real_draws(pkg, oracle_lib, gpu_engine):
    for n in (1037, 16421):
        x = _block(pkg, oracle_lib, "real", n)
        cases.check_center(x, x[0])
        cases.check_moments(gpu_engine.pool_joint(x), ref.moments(x, x[0]), f"moments real draws n={n}")


def test_moments_of_a_trace_block_are_those_of_its_rows(gpu_engine):
    x = cases.synthetic(1037 * 3, 3)
    assert np.array_equal(gpu_engine.pool_joint_partials(x.reshape(1037, 3, 3)), gpu_engine.pool_joint_partials(x))


@pytest.mark.parametrize("d", [3, 8])
def test_moment_shards_add(gpu_engine, d):
    x = cases.synthetic(16421, d)
    c = cases.given_center(x)
    cases.check_center(x, c)
    parts = gpu_engine.pool_joint_partials(x[:5000], c) + gpu_engine.pool_joint_partials(x[5000:], c)
    assert parts[0] == 16421 and parts[1] == 0
    cases.check_moments(gpu_engine.pool_joint_finish(parts, c), ref.moments(x, c), f"two uneven shards d={d}")


@pytest.mark.parametrize("d", [2, 3, 8])
def test_moments_leave_out_non_finite_rows(gpu_engine, d):
    x = cases.synthetic(1037, d).copy()
    x[3, d - 1], x[17, 0], x[700, 1], x[1030, 0] = np.nan, np.inf, -np.inf, np.nan
    x[1030, 1] = np.inf
    c = x[0]
    got = gpu_engine.pool_joint(x, c)
    assert got["nonfinite"] == 4 and got["n"] == 1033
    keep = np.isfinite(x).all(axis=1)
    cases.check_moments(got, ref.moments(x[keep], c), f"non-finite rows d={d}")


def test_moments_degenerate(pkg, gpu_engine):
    x = cases.synthetic(5, 3)
    one = gpu_engine.pool_joint(x[:1])
    assert one["n"] == 1 and np.array_equal(one["mean"], x[0]) and np.isnan(one["cov"]).all() and np.isnan(one["corr"]).all()
    z = cases.synthetic(1037, 3).copy()
    z[:, 1] = 0.011
    corr = gpu_engine.pool_joint(z)["corr"]
    assert np.isnan(corr[1]).all() and np.isnan(corr[:, 1]).all() and corr[0, 0] == 1.0 and np.isfinite(corr[0, 2])
    with pytest.raises(pkg._abi.RsfError):
        gpu_engine.pool_joint_partials(x, [np.nan, 0.0, 0.0])
    with pytest.raises(ValueError):
        gpu_engine.pool_joint_partials(np.zeros((4, 9)))


# ---- 2-D KDE ---------------------------------------------------------------------------------------------------------

def _points(x2, which):
    if which == "one":
        return x2.mean(0).reshape(1, 2) + 0.3 * x2.std(0)
    if which == "mesh63":
        return cases.mesh(x2, 8.0, 9, 7)
    if which == "m1031":
        return cases.scattered(x2, 1031, 5)
    assert which == "chunk+1"
    return cases.scattered(x2, CHUNK + 1, 6)


@pytest.mark.parametrize("which", ["one", "mesh63", "m1031", "chunk+1"])
@pytest.mark.parametrize("n", cases.SIZES)
def test_kde2d_synthetic(gpu_engine, n, which):
    x = cases.synthetic(n, 3)
    # (the long-double reference of 16 421 draws at a thousand points takes seconds: one pair each there)
    pairs = cases.PAIRS3 if which in ("mesh63", "one") or n <= 1037 else {"m1031": ((0, 1),), "chunk+1": ((2, 0),)}[which]
    for pair in pairs:
        x2 = np.ascontiguousarray(x[:, list(pair)])
        pts = _points(x2, which)
        want = _kde_ref(("syn", n, pair, which), x2, pts)
        got = gpu_engine.pool_kde2d(x, pts, params=pair)
        assert got.shape == (pts.shape[0],)
        cases.check_kde(got, want, f"kde2d synthetic n={n} pair={pair} m={pts.shape[0]}")
        if which == "mesh63":
            assert (want < cases.KDE_FLOOR).any() or n <= 5, "the mesh is meant to run past underflow"


@pytest.mark.parametrize("n", [1037, 16421])
def test_kde2d_real_draws(pkg, oracle_lib, gpu_engine, n):
    x = _block(pkg, oracle_lib, "real", n)
    for pair, which in (((0, 1), "m1031"), ((1, 2), "mesh63"), ((2, 0), "one")) if n == 1037 else (((0, 2), "chunk+1"), ((2, 1), "mesh63")):
        x2 = np.ascontiguousarray(x[:, list(pair)])
        pts = _points(x2, which)
        cases.check_kde(gpu_engine.pool_kde2d(x, pts, params=pair), _kde_ref(("real", n, pair, which), x2, pts),
                        f"kde2d real draws n={n} pair={pair} m={pts.shape[0]}")


def test_kde2d_two_columns_device_memory_and_twice(gpu_engine, dev_engine):
    import torch

    x = cases.synthetic(1037, 3)
    x2 = np.ascontiguousarray(x[:, :2])
    pts = _points(x2, "m1031")
    want = _kde_ref(("syn", 1037, (0, 1), "m1031"), x2, pts)
    got = gpu_engine.pool_kde2d(x2, pts)  # a d = 2 block
    cases.check_kde(got, want, "kde2d d=2 block")
    assert np.array_equal(got, gpu_engine.pool_kde2d(x2, pts)), "two calls differ"
    assert np.array_equal(got, gpu_engine.pool_kde2d(x, pts, params=(0, 1))), "the d = 2 block and columns (0, 1) of the d = 3 block differ"
    dens = dev_engine.pool_kde2d(torch.as_tensor(x2, device="cuda"), torch.as_tensor(pts, device="cuda"))
    assert dens.is_cuda and np.array_equal(dens.cpu().numpy(), got)
    # the reversed pair is the same density at the swapped points (another factorisation: to rounding)
    rev = gpu_engine.pool_kde2d(x, pts[:, ::-1].copy(), params=(1, 0))
    cases.check_kde(rev, want, "kde2d reversed pair (1, 0)")


def test_kde2d_bandwidth_given(gpu_engine):
    x = cases.synthetic(1037, 3)
    x2 = np.ascontiguousarray(x[:, [0, 2]])
    pts = _points(x2, "mesh63")
    for bw in (0.11, 0.8):
        cases.check_kde(gpu_engine.pool_kde2d(x, pts, params=(0, 2), bw_factor=bw), ref.kde2d(x2, pts, bw_factor=bw), f"kde2d bw_factor={bw}")


def test_kde2d_shards_add(gpu_engine):
    n = 16421
    x = cases.synthetic(n, 3)
    pair = (0, 1)
    x2 = np.ascontiguousarray(x[:, list(pair)])
    pts = _points(x2, "m1031")
    whole = gpu_engine.pool_kde2d(x, pts, params=pair)
    cov = gpu_engine.pool_joint(x)["cov"][np.ix_(pair, pair)]
    parts = sum(gpu_engine.pool_kde2d(s, pts, params=pair, cov=cov, n_total=n) for s in (x[:1000], x[1000:9001], x[9001:]))
    rel = np.abs(parts - whole) / whole
    print(f"kde2d three uneven shards against one call: largest relative difference {rel.max():.3e}")
    assert np.all(rel <= cases.RTOL_SHARDS)
    cases.check_kde(parts, _kde_ref(("syn", n, pair, "m1031"), x2, pts), "kde2d sum of three shards")
    # ... and with cov= and n_total= of the block itself, the call without them (the library's own moments, to rounding)
    same = gpu_engine.pool_kde2d(x, pts, params=pair, cov=cov, n_total=n)
    assert np.all(np.abs(same - whole) <= cases.RTOL_SHARDS * whole)


def test_kde2d_slices_of_more_than_one_tile(gpu_engine):
    """n = 2^20 + 1 (joint_cases.N_MULTI_TILE): the first sizes at which a slice of pool_kde2d_kernel streams more than one tile."""
    n = cases.N_MULTI_TILE
    x = _block(None, None, "synthetic", n, 3)
    pair = (0, 1)
    x2 = np.ascontiguousarray(x[:, list(pair)])
    one = _points(x2, "one")
    cases.check_kde(gpu_engine.pool_kde2d(x, one, params=pair), _kde_ref(("syn", n, pair, "one"), x2, one), f"kde2d n={n} m=1: 1024 slices of 1025")
    pts = _points(x2, "m1031")
    got = gpu_engine.pool_kde2d(x, pts, params=pair)
    assert got.shape == (1031,) and np.isfinite(got).all() and np.all(got >= 0)
    idx = [0, 255, 1024, 1030]   # the first chunk's first and second register point, the second chunk's first and last thread
    want = _kde_ref(("syn", n, pair, "m1031", tuple(idx)), x2, pts[idx])
    cases.check_kde(got[idx], want, f"kde2d n={n} m=1031 (512 slices of 2049, three tiles each), points {idx}")


def test_kde2d_refuses(pkg, gpu_engine):
    x = cases.synthetic(1037, 3).copy()
    pts = x[:4, :2].copy()
    line = x.copy()
    line[:, 1] = 2.0 * line[:, 0]
    with pytest.raises(pkg._abi.RsfError, match="singular KDE"):
        gpu_engine.pool_kde2d(line, pts, params=(0, 1))
    line[:, 2] = 3.0 * line[:, 0] + 1.0
    with pytest.raises(pkg._abi.RsfError, match="singular KDE"):
        gpu_engine.pool_kde2d(line, pts, params=(2, 0))
    with pytest.raises(pkg._abi.RsfError, match="singular KDE"):
        gpu_engine.pool_kde2d(x, pts, cov=[[1.0, 2.0], [2.0, 1.0]])
    with pytest.raises(pkg._abi.RsfError, match="singular KDE"):
        gpu_engine.pool_kde2d(x, pts, cov=[[1.0, 0.0], [0.0, np.nan]])
    with pytest.raises(ValueError):
        gpu_engine.pool_kde2d(x, pts, params=(1, 1))
    with pytest.raises(ValueError):
        gpu_engine.pool_kde2d(x, pts, params=(0, 3))
    with pytest.raises(pkg._abi.RsfError):
        gpu_engine.pool_kde2d(x[:2], pts)
    with pytest.raises(pkg._abi.RsfError):  # pa == pb through the C ABI itself
        dens = np.empty(4)
        pkg._abi.check(gpu_engine.lib, gpu_engine.lib.rsf_pool_kde2d(gpu_engine._ctx, 1037, 3, x.ctypes.data, 1, 1, 4, pts.ctypes.data, 0.0,
                                                                      None, 0, dens.ctypes.data))
    with pytest.raises(pkg._abi.RsfError):
        gpu_engine.pool_kde2d(x, pts, n_total=5)
    assert gpu_engine.pool_kde2d(x[:3], pts).shape == (4,)  # n = 3 is the smallest


# ---- 2-D histogram ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbins", [(1, 1), (20, 16), (126, 126)])
def test_histogram2d_edge_block(gpu_engine, dev_engine, nbins):
    import torch

    nbx, nby = nbins
    x, ranges = cases.edge_block(16421, nbx, nby, 21)
    (lo_a, hi_a), (lo_b, hi_b) = ranges
    want = ref.hist2d(x[:, 0], x[:, 2], nbx, nby, lo_a, hi_a, lo_b, hi_b)
    got = gpu_engine.pool_histogram2d(x, nbins, ranges, params=(0, 2))
    assert got.shape == (nbx + 2, nby + 2) and got.sum() == x.shape[0]
    assert np.array_equal(got, want)
    assert got[0].sum() > 0 and got[-1].sum() > 0 and got[:, 0].sum() > 0 and got[:, -1].sum() > 0  # the border is exercised
    dev = dev_engine.pool_histogram2d(torch.as_tensor(x, device="cuda"), nbins, ranges, params=(0, 2))
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    # two shards add exactly; the transposed pair is the transposed table
    a = gpu_engine.pool_histogram2d(x[:6000], nbins, ranges, params=(0, 2))
    b = gpu_engine.pool_histogram2d(x[6000:], nbins, ranges, params=(0, 2))
    assert np.array_equal(a + b, want)
    t = gpu_engine.pool_histogram2d(x, (nby, nbx), ranges[::-1], params=(2, 0))
    assert np.array_equal(t, want.T)


@pytest.mark.parametrize("n", cases.SIZES_CAPPED)
def test_histogram2d_past_the_grid_cap(gpu_engine, n):
    nbx, nby = 20, 16
    x, ranges = cases.edge_block(n, nbx, nby, 23)
    got = gpu_engine.pool_histogram2d(x, (nbx, nby), ranges, params=(0, 2))
    assert got.shape == (nbx + 2, nby + 2) and got.sum() == n
    fin = np.isfinite(x[:, 0]) & np.isfinite(x[:, 2])
    assert np.array_equal(got[1:-1, 1:-1], np.histogram2d(x[fin, 0], x[fin, 2], (nbx, nby), ranges)[0])
    assert np.array_equal(got, ref.hist2d(x[:, 0], x[:, 2], nbx, nby, *ranges[0], *ranges[1]))
    assert got[0].sum() > 0 and got[-1].sum() > 0 and got[:, 0].sum() > 0 and got[:, -1].sum() > 0


def test_histogram2d_blocks_and_int_nbins(pkg, oracle_lib, gpu_engine):
    for kind in ("synthetic", "real"):
        x = _block(pkg, oracle_lib, kind, 16421)
        for pair in ((0, 1), (1, 2)):
            a, b = x[:, pair[0]], x[:, pair[1]]
            ranges = ((a.min(), a.max()), (b.min(), b.max()))
            got = gpu_engine.pool_histogram2d(x, 40, ranges, params=pair)
            want = ref.hist2d(a, b, 40, 40, *ranges[0], *ranges[1])
            assert np.array_equal(got, want) and got[1:-1, 1:-1].sum() == 16421
            assert np.array_equal(got[1:-1, 1:-1], np.histogram2d(a, b, 40, ranges)[0])
    small = cases.synthetic(3, 2)
    assert gpu_engine.pool_histogram2d(small, 4, ((990.0, 1010.0), (0.0, 1.0))).sum() == 3


def test_histogram2d_refuses(pkg, gpu_engine):
    x = cases.synthetic(1037, 3)
    ok = ((990.0, 1010.0), (0.0, 1.0))
    with pytest.raises(pkg._abi.RsfError, match="16384"):
        gpu_engine.pool_histogram2d(x, (127, 127), ok)
    with pytest.raises((pkg._abi.RsfError, ValueError)):
        gpu_engine.pool_histogram2d(x, 0, ok)
    with pytest.raises(pkg._abi.RsfError):  # nbins = 0 through the C ABI itself
        out = np.empty(64)
        pkg._abi.check(gpu_engine.lib, gpu_engine.lib.rsf_pool_histogram2d(gpu_engine._ctx, 1037, 3, x.ctypes.data, 0, 1, 0, 0.0, 1.0, 4, 0.0, 1.0,
                                                                            out.ctypes.data))
    for bad in (((1.0, 1.0), (0.0, 1.0)), ((0.0, 1.0), (2.0, 1.0)), ((0.0, np.inf), (0.0, 1.0)), ((0.0, 1.0), (np.nan, 1.0))):
        with pytest.raises(pkg._abi.RsfError):
            gpu_engine.pool_histogram2d(x, 8, bad)
    with pytest.raises(ValueError):
        gpu_engine.pool_histogram2d(x, 8, ok, params=(2, 2))
    assert gpu_engine.pool_histogram2d(x, (126, 126), ok).shape == (128, 128)  # the limit itself


# ---- highest-density levels ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.HPD_CASES))
def test_hpd_levels_hand_made(gpu_engine, name):
    w, probs, want = cases.HPD_CASES[name]
    assert np.array_equal(gpu_engine.pool_hpd_levels(w, probs), np.array(want))
    assert np.array_equal(gpu_engine.pool_hpd_levels(w, probs), ref.hpd_levels(w, probs))


def test_hpd_levels_of_a_histogram(pkg, gpu_engine):
    x = cases.synthetic(16421, 3)
    a, b = x[:, 0], x[:, 1]
    counts = gpu_engine.pool_histogram2d(x, (20, 16), ((a.min(), a.max()), (b.min(), b.max())))[1:-1, 1:-1]
    probs = (0.1, 0.5, 0.683, 0.9, 0.99)
    levels = gpu_engine.pool_hpd_levels(counts, probs)
    assert np.array_equal(levels, ref.hpd_levels(counts, probs)) and np.all(np.diff(levels) <= 0)
    for p, lv in zip(probs, levels):
        assert counts[counts >= lv].sum() >= p * 16421 and counts[counts > lv].sum() < p * 16421
    for bad in ([1.0, -1.0], [np.nan, 1.0], [0.0, 0.0], [np.inf, 1.0]):
        with pytest.raises(pkg._abi.RsfError):
            gpu_engine.pool_hpd_levels(bad, (0.5,))
    for p in (0.0, 1.0, np.nan):
        with pytest.raises(pkg._abi.RsfError):
            gpu_engine.pool_hpd_levels([1.0, 2.0], (p,))


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_pool_joint_and_corner_end_to_end(pkg, cpu_engine):
    """A small joint (Dc, a, b) run of MCMC.sample_batched, in the recipe of tests/test_gpu_posterior.py's d = 3 case."""
    from conftest import synthetic_data

    model = pkg.RateStateModel(number_time_steps=500)
    model.RadiationDamping = True
    cpu_engine.set_model(model, 1)
    data = synthetic_data(cpu_engine)
    lo, hi = [0.0, 0.005, 0.005], [1.0e4, 0.02, 0.03]
    mc = pkg.MCMC(model, data, 1000.0, [["Uniform", a, b] for a, b in zip(lo, hi)], [1600.0, 0.008, 0.022], nsamples=200, verbose=False)
    mc.n0 = 0.0
    pool = mc.sample_batched(512, seed=2026, mem="host")
    q = pool.pooled()  # (3, n)
    n = q.shape[1]
    j = pool.joint()
    assert j["n"] == n and j["nonfinite"] == 0
    first = np.asarray(pool.samples).reshape(-1, 3)[0]
    cases.check_center(q.T, first)
    cases.check_moments(j, ref.moments(q.T, first), "end to end: pool.joint()")
    sd = np.sqrt(np.diag(np.cov(q)))
    assert np.all(np.abs(j["cov"] - np.cov(q)) <= cases.TOL_COV * np.outer(sd, sd))
    probs = (0.5, 0.9)
    res = pool.corner(nbins=12, grid=8, probs=probs)
    assert set(res) == {"joint", "ranges", "probs", "marginals", "pairs"} and set(res["pairs"]) == {(0, 1), (0, 2), (1, 2)}
    assert res["ranges"].shape == (3, 2) and np.array_equal(res["joint"]["cov"], j["cov"]) and len(res["marginals"]) == 3
    for p, mg in enumerate(res["marginals"]):
        assert mg["counts"].shape == (12,) and mg["edges"].shape == (13,) and mg["grid"].shape == (8,) and mg["density"].shape == (8,)
        assert mg["counts"].sum() == n and np.isfinite(mg["density"]).all()
        assert np.array_equal(mg["counts"], np.histogram(q[p], 12, tuple(res["ranges"][p]))[0])
    for (a, b), pr in res["pairs"].items():
        assert set(pr) == {"counts", "xedges", "yedges", "x", "y", "density", "levels"}
        assert pr["counts"].shape == (12, 12) and pr["xedges"].shape == (13,) and pr["yedges"].shape == (13,)
        assert pr["density"].shape == (8, 8) and pr["x"].shape == (8,) and pr["y"].shape == (8,) and pr["levels"].shape == (2,)
        assert pr["counts"].sum() == n, "the default ranges are min and max: every draw is inside"
        h, xe, ye = np.histogram2d(q[a], q[b], 12, (tuple(res["ranges"][a]), tuple(res["ranges"][b])))
        assert np.array_equal(pr["counts"], h) and np.array_equal(pr["xedges"], xe) and np.array_equal(pr["yedges"], ye)
        assert np.isfinite(pr["density"]).all() and (pr["density"] >= 0).all() and pr["density"].max() > 0
        assert np.all(np.diff(pr["levels"]) <= 0)
        # density[k, l] is at (x[k], y[l])
        k, l = np.unravel_index(np.argmax(pr["density"]), (8, 8))
        one = ref.kde2d(np.ascontiguousarray(q[[a, b]].T), np.array([[pr["x"][k], pr["y"][l]]]))
        assert abs(pr["density"][k, l] - float(one[0])) <= cases.RTOL_KDE * float(one[0])
