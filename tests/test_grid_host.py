"""
CPU tests of the grid posterior's host side: the prototype table, rsf_grid_finish (host only: no ctx, no GPU) against the
long-double specification (tests/grid_reference.py) on crafted column fields, its argument checks — rsfh::grid_check, the check
every rsf_grid_* entry point begins with — the grid without a finite node, and the argument errors the Python layer raises
before any library call.
"""
import ctypes

import numpy as np
import pytest

import grid_reference as G

ERR_INVALID = -1
TOL = 1e-12  # the project's bound for scaled sums


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _finish(lib, x, w, coords, center, shape, lo, hi, lmax, fields, n=None, null=None):
    """rsf_grid_finish through ctypes → (rc, dict)"""
    d = len(x)
    n = np.array([a.size for a in x] if n is None else n, dtype=np.int32)
    n1, n2 = (x[1].size if d > 1 else 1), (x[2].size if d > 2 else 1)
    xc, wc = np.concatenate(x), np.concatenate(w)
    lo, hi, f = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64), np.ascontiguousarray(fields, dtype=np.float64)
    out = {"head": np.empty(20), "mass1": np.empty(n1), "mass2": np.empty(n2), "pair": np.empty((n2, n1)), "cum1": np.empty((n2, n1)), "cum2": np.empty(n2)}
    args = [d, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _dp(xc), _dp(wc), coords, center, shape, _dp(lo), _dp(hi), lmax, _dp(f)] + [_dp(v) for v in out.values()]
    if null is not None:
        args[null] = None
    return lib.rsf_grid_finish(*args), out


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._abi.load()


def test_prototype_table(pkg, lib):
    abi = pkg._abi
    assert sorted(abi.GRID_PROTOTYPES) == ["rsf_grid_cdf", "rsf_grid_columns", "rsf_grid_draw", "rsf_grid_finish", "rsf_grid_logtarget"]
    assert [len(abi.GRID_PROTOTYPES[k][1]) for k in sorted(abi.GRID_PROTOTYPES)] == [10, 12, 13, 17, 11]
    assert all(rt is ctypes.c_int for rt, _ in abi.GRID_PROTOTYPES.values())
    for name, (_, argtypes) in abi.GRID_PROTOTYPES.items():
        assert list(getattr(lib, name).argtypes) == argtypes, name
    assert abi.GRID_HEAD == 20 and len(abi.GRID_FIELDS) == G.FIELDS and (abi.GRID_PLAIN, abi.GRID_PRODUCT) == (G.PLAIN, G.PRODUCT)
    assert {"GridPosterior"} <= set(pkg.__all__)


def _crafted(shape_n, seed, coords):
    """a grid with uneven nodes, l spread over 1e4 with one column and one node without density, and the fields of the specification"""
    rng = np.random.default_rng(seed)
    x = [np.sort(rng.uniform(1.0, 3.0, n)) + 0.5 * p for p, n in enumerate(shape_n)]
    w = [rng.uniform(0.5, 1.5, n) / n for n in shape_n]
    N = int(np.prod(shape_n))
    l = rng.uniform(-1e4, 0.0, N)
    l[rng.integers(0, N, N // 3)] = rng.uniform(-30.0, 0.0, N // 3)
    ssq = rng.uniform(0.5, 2.0, N)
    if len(shape_n) > 1:
        l[shape_n[0]:2 * shape_n[0]] = -np.inf  # column 1
    l[N - 1] = -np.inf
    center = float(x[0][shape_n[0] // 2])
    col = G.columns(x, w, l, ssq, center)
    return x, w, center, col, l, ssq


@pytest.mark.parametrize("shape_n,coords", [((5,), G.PLAIN), ((17, 4), G.PLAIN), ((33, 5, 3), G.PLAIN), ((33, 5, 3), G.PRODUCT), ((257, 9, 7), G.PRODUCT)])
def test_finish_against_the_specification(lib, shape_n, coords):
    x, w, center, col, _, _ = _crafted(shape_n, 11, coords)
    d = len(shape_n)
    lo, hi, shape = [0.5] * d, [10.0] * d, 7.5
    want = G.finish(x, w, coords, center, shape, lo, hi, col["lmax"], col["fields"])
    rc, got = _finish(lib, x, w, coords, center, shape, lo, hi, col["lmax"], col["fields"].astype(np.float64))
    assert rc == 0, lib.rsf_last_error()
    h = got["head"]
    worst = 0.0

    def close(name, a, b, scale=None):
        nonlocal worst
        a, b = np.asarray(a, dtype=G.LD), np.asarray(b, dtype=G.LD)
        s = np.abs(b).max() if scale is None else scale
        err = float(np.abs(a - b).max() / s)
        worst = max(worst, err)
        assert err < TOL, f"{name}: {err:.2e}"

    close("Z", h[0], want["Z"])
    close("log_integral", h[1], want["log_integral"])
    close("log_evidence", h[2], want["log_evidence"])
    assert h[3] == want["n_neginf"]
    # the scale of a moment's sums: the spans of the axes (of q0 = x0 / x1 in product coordinates)
    q = G.nodes(x, coords)
    sd = q.max(axis=0) - q.min(axis=0)
    for p in range(d):
        close(f"mean {p}", h[4 + p], want["mean"][p], sd[p])
        for r in range(d):
            close(f"cov {p}{r}", h[7 + 3 * p + r], want["cov"][p, r], sd[p] * sd[r])
    assert np.isnan(h[4 + d:7]).all()
    close("x0 mean", h[16], want["x0_mean"], np.ptp(x[0]))
    close("x0 var", h[17], want["x0_var"], np.ptp(x[0]) ** 2)
    close("std2 mean", h[18], want["std2_mean"])
    close("std2 var", h[19], want["std2_var"], float(want["std2_mean"]) ** 2)
    for k in ("pair", "mass1", "mass2", "cum1", "cum2"):
        close(k, got[k], np.asarray(want[k]).reshape(got[k].shape), 1.0)
    print(f"{shape_n} coords {coords}: worst scaled error {worst:.2e}")
    assert got["cum1"][0, -1] == 1.0 if d > 1 else got["cum1"][0, 0] == 0.0
    if d > 1:
        assert not got["pair"][0, 1] and not got["cum1"].min() < 0


def test_every_node_without_density(lib):
    x, w = [np.linspace(0.0, 1.0, 5), np.linspace(1.0, 2.0, 3)], [np.full(5, 0.25), np.full(3, 0.5)]
    fields = np.zeros((3, 6))
    fields[:, 5] = 5
    rc, got = _finish(lib, x, w, G.PLAIN, 0.5, 4.0, [0.0, 1.0], [1.0, 2.0], -np.inf, fields)
    assert rc == 0
    h = got["head"]
    assert h[1] == -np.inf and h[3] == 15 and np.isnan(np.delete(h, [1, 3])).all()
    assert all(np.isnan(got[k]).all() for k in ("mass1", "mass2", "pair", "cum1", "cum2"))


def test_finish_argument_checks(lib):
    x, w = [np.linspace(1.0, 2.0, 5), np.linspace(1.0, 2.0, 3), np.linspace(1.0, 2.0, 3)], [np.full(5, 0.2), np.full(3, 0.5), np.full(3, 0.5)]
    fields, box = np.ones((9, 6)), ([0.5] * 3, [3.0] * 3)
    ok = lambda **kw: _finish(lib, kw.pop("x", x), kw.pop("w", w), kw.pop("coords", G.PRODUCT), kw.pop("center", 1.5), kw.pop("shape", 4.0),
                              kw.pop("lo", box[0]), kw.pop("hi", box[1]), kw.pop("lmax", 0.0), kw.pop("fields", fields), **kw)[0]
    assert ok() == 0
    big = [np.linspace(1.0, 2.0, m) for m in (2048, 1024, 1024)]
    bad = [dict(n=[5, 1, 3]), dict(x=big, w=big),                                                   # sizes: an axis of one node, 2^31 nodes
           dict(x=[x[0][::-1].copy(), x[1], x[2]]), dict(x=[x[0], np.array([1.0, 1.0, 2.0]), x[2]]),  # unsorted, repeated nodes
           dict(x=[x[0], x[1], np.array([1.0, np.nan, 2.0])]),
           dict(w=[w[0], np.array([0.5, 0.0, 0.5]), w[2]]), dict(w=[w[0], w[1], np.array([0.5, -1.0, 0.5])]), dict(w=[np.full(5, np.inf), w[1], w[2]]),
           dict(coords=2), dict(lo=[0.5, 0.0, 0.5]), dict(lo=[0.5, 3.0, 0.5]), dict(shape=0.0), dict(shape=np.nan), dict(center=np.inf),
           dict(lmax=np.nan), dict(lmax=np.inf)]
    bad += [dict(null=k) for k in (1, 2, 3, 7, 8, 10, 11, 12, 13, 14, 15, 16)]                      # NULL pointers
    for kw in bad:
        assert ok(**kw) == ERR_INVALID, kw
        assert b"rsf_grid_finish" in lib.rsf_last_error()
    # PRODUCT needs d = 3; d outside 1..3
    assert _finish(lib, x[:2], w[:2], G.PRODUCT, 1.5, 4.0, box[0][:2], box[1][:2], 0.0, np.ones((3, 6)))[0] == ERR_INVALID
    assert _finish(lib, x[:2], w[:2], G.PLAIN, 1.5, 4.0, box[0][:2], box[1][:2], 0.0, np.ones((3, 6)))[0] == 0
    n = np.array([5, 3, 3, 3], dtype=np.int32)
    d4 = [4, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))] + [_dp(np.ones(16))] * 2 + [0, 1.5, 4.0] + [_dp(np.ones(4))] * 2 + [0.0] + [_dp(np.ones(64))] * 7
    assert lib.rsf_grid_finish(*d4) == ERR_INVALID


def test_python_layer_argument_errors(pkg, cpu_engine):
    """raised before any library call: the checker's library has no rsf_grid_* at all"""
    eng = cpu_engine
    eng.set_model(pkg.RateStateModel(number_time_steps=50), 1)
    data, x = np.zeros(eng.nout), np.linspace(1.0, 2.0, 5)
    with pytest.raises(ValueError, match="1 to 3 axes"):
        eng.grid_logtarget([x] * 4, data, [0.0] * 4, [1.0] * 4)
    with pytest.raises(ValueError, match="as many weights"):
        eng.grid_columns([x], [np.ones(4)], np.zeros(5), np.ones(5))
    with pytest.raises(ValueError, match="coords"):
        eng.grid_logtarget([x], data, 0.0, 3.0, coords="product")
    with pytest.raises(ValueError, match="coords"):
        eng.grid_logtarget([x], data, 0.0, 3.0, coords="polar")
    with pytest.raises(ValueError, match="data has shape"):
        eng.grid_logtarget([x], data[:-1], 0.0, 3.0)
    with pytest.raises(ValueError, match="one value per node"):
        eng.grid_columns([x], [np.ones(5)], np.zeros(4), np.ones(4))
    with pytest.raises(ValueError, match="odd node counts"):
        eng.grid_posterior(data, 0.0, 1e4, n=(4000,))
    with pytest.raises(ValueError, match="odd node counts"):
        eng.grid_posterior(data, [0.0, 0.005, 0.005], [1e4, 0.02, 0.03], n=(2001, 65))
    with pytest.raises(ValueError, match="d = 1"):
        eng.grid_posterior(data, [0.0, 0.005], [1e4, 0.02])
    with pytest.raises(ValueError, match="cum1 is"):
        eng.grid_draw([x, x], np.zeros(25), np.zeros(4), None, 8)


def test_dc_cdf_refines_a_uniform_a_axis_only(pkg):
    """GridPosterior.dc_cdf through a stub engine whose grid_cdf is the specification's: Gauss-Legendre axes and sub = 1 take the
    grid as it is; a uniform a axis is refined four times, in slabs of axis-2 nodes, and gives a proper CDF"""
    import posterior_reference as R

    calls = []

    class Stub:
        def grid_cdf(self, x, cum0, pair, xs, coords):
            calls.append(tuple(a.size for a in x))
            return np.asarray(G.cdf(x, coords, np.asarray(cum0), pair, xs), dtype=np.float64)

    c = R.CLOSED[3]
    fn = R.quadratic_ssq(c["S0"], c["q0"], c["K"])

    def post(rule):
        ax = [G.simpson(1.2, 3.0, 401)] + [rule(c["lo"][p], c["hi"][p], 17) for p in (1, 2)]
        x, w = [a[0] for a in ax], [a[1] for a in ax]
        col, fin, _, _ = G.posterior(fn, x, w, c["lo"], c["hi"], c["shape"], G.PRODUCT, dtype=np.float64)
        fin = {k: (np.asarray(v, dtype=np.float64) if hasattr(v, "shape") else float(v)) for k, v in fin.items()}
        return pkg.GridPosterior(Stub(), x, w, G.PRODUCT, np.array(c["lo"]), np.array(c["hi"]), c["shape"], col, fin, None, 0.0, 0)

    xs = np.linspace(0.3, 2.5, 201)
    gl = post(G.gauss_legendre)
    F = gl.dc_cdf(xs)
    assert calls == [(401, 17, 17)]  # not uniform: one call on the grid itself
    np.testing.assert_array_equal(F, Stub().grid_cdf(gl.x, gl.cum0, gl.finish["pair"], xs, G.PRODUCT))
    un = post(G.simpson)
    del calls[:]
    plain = un.dc_cdf(xs, sub=1)
    assert calls == [(401, 17, 17)]
    del calls[:]
    fine = un.dc_cdf(xs)
    assert len(calls) == 3 and all(n[:2] == (401, 65) for n in calls) and sum(n[2] for n in calls) == 17  # slabs of axis-2 nodes
    assert fine[0] == 0.0 and abs(fine[-1] - 1.0) < 1e-12 and (np.diff(fine) > -1e-12).all()
    print(f"refined against plain: {np.abs(fine - plain).max():.2e}")  # the accuracy is tests/test_gpu_grid.py's, against the reference


def test_dc_cdf_against_the_closed_reference(pkg):
    """the accuracy of the refined sum without a GPU: GridPosterior.dc_cdf over the specification's cdf (a stub engine) on the
    d = 3 closed form, (2001, 33, 33) Simpson nodes in product coordinates on the reference's window.  Dc's five quantiles within
    0.25 Monte-Carlo SE at C = 262 144 of closed_reference(3)'s, the margin tests/test_gpu_grid.py holds the real model to."""
    import posterior_reference as R

    class Stub:
        def grid_cdf(self, x, cum0, pair, xs, coords):
            return np.asarray(G.cdf(x, coords, np.asarray(cum0), pair, xs), dtype=np.float64)

    ref, fn, c = R.closed_reference(3)
    ax = [G.simpson(ref.plo, ref.phi, 2001)] + [G.simpson(c["lo"][p], c["hi"][p], 33) for p in (1, 2)]
    x, w = [a[0] for a in ax], [a[1] for a in ax]
    col, fin, _, _ = G.posterior(fn, x, w, c["lo"], c["hi"], c["shape"], G.PRODUCT, dtype=np.float64)
    fin = {k: (np.asarray(v, dtype=np.float64) if hasattr(v, "shape") else float(v)) for k, v in fin.items()}
    post = pkg.GridPosterior(Stub(), x, w, G.PRODUCT, np.array(c["lo"]), np.array(c["hi"]), c["shape"], col, fin, None, 0.0, 0)
    shift = np.abs(post.quantiles("Dc", R.PROBS) - ref.marg["Dc"].quantiles()) / R.se_table(ref, 262144)["Dc"]["q"]
    print(f"Dc quantiles, refined sum at 33 a nodes: {shift.max():.3f} SE")
    assert shift.max() < 0.25
