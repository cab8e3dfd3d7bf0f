"""
GPU tests of the exact posterior on a tensor quadrature grid (include/rsf_grid.h) against its specification
(tests/grid_reference.py), the evidence kernel, the CPU checker and the reference quadrature (tests/posterior_reference.py).

Bounds.  The fused kernel's l: the bits of rsf_evidence_logtarget on the same points in the same order (the same arrangement, so
the per-wave tier decisions are the same); its ssq: 1e-9 relative of the checker, the project's bound for a float64 RK4 solve.
Product coordinates: Dc = x0 / x1 is one IEEE division, the one NumPy makes, and l + log x1 differs from the evidence kernel's
-shape log SSq by the rounding of one fused multiply-add and one logarithm: 4 ulp of |l|.  Reductions: 1e-12 of the scale of each
sum, the project's bound for scaled sums.  Draws: the thresholds of posterior_reference.check.  Real model: shape 1e-9 on log I
(l = -shape log SSq, SSq within 1e-9); a weight perturbation of eps moves the mean by at most eps SD, so 4 shape 1e-9.
"""
import json
import os

import numpy as np
import pytest

import grid_reference as G
import posterior_reference as R
from conftest import GOLDEN
from test_gpu_posterior import BOX1, HI3, LO3, _model, _reference
from test_grid_host import _crafted

pytestmark = pytest.mark.gpu

TOL = 1e-12
N_DRAWS = 262144


def _setup(pkg, gpu_engine, cpu_engine, damping=True, substeps=1, nsteps=500):
    cpu_engine.set_model(_model(pkg, nsteps), 1)
    from conftest import synthetic_data
    data = synthetic_data(cpu_engine)
    for e in (gpu_engine, cpu_engine):
        e.set_model(_model(pkg, nsteps, damping=damping), substeps)
    return data


def _checker_ssq(cpu_engine, data, q):
    q = np.asarray(q).reshape(len(q), -1)
    kw = {} if q.shape[1] == 1 else dict(a=np.ascontiguousarray(q[:, 1]), b=np.ascontiguousarray(q[:, 2]))
    ssq, _ = cpu_engine.forward(np.ascontiguousarray(q[:, 0]), data=data, want_ssq=True, want_acc=False, **kw)
    return np.asarray(ssq)


def _plain_axes(d):
    """interior nodes; (129, 5, 3) is 1935 nodes: a partial last wave, waves that straddle columns"""
    if d == 1:
        return [np.linspace(150.0, 4000.0, 193)], [BOX1[0]], [BOX1[1]]
    return [np.linspace(300.0, 3000.0, 129), np.linspace(0.006, 0.019, 5), np.linspace(0.008, 0.028, 3)], LO3, HI3


@pytest.mark.parametrize("d,damping,substeps", [(3, True, 1), (3, False, 1), (1, True, 1), (1, False, 1), (3, True, 8)])
def test_fused_kernel_plain(pkg, gpu_engine, cpu_engine, d, damping, substeps):
    """grid_logtarget_kernel<D, DAMP, PLAIN>; substeps 8: the loading table is staged in two chunks"""
    data = _setup(pkg, gpu_engine, cpu_engine, damping, substeps)
    x, lo, hi = _plain_axes(d)
    l, ssq = (np.asarray(v) for v in gpu_engine.grid_logtarget(x, data, lo, hi))
    q = G.nodes(x)
    want = np.asarray(gpu_engine.evidence_logtarget(q, data, lo, hi, np.zeros(len(q))))
    assert np.isfinite(l).all()
    np.testing.assert_array_equal(l.view(np.int64), want.view(np.int64))
    ref = _checker_ssq(cpu_engine, data, q)
    err = np.abs(ssq / ref - 1.0).max()
    print(f"d = {d} damping {damping} substeps {substeps}: {len(q)} nodes, ssq against the checker {err:.2e}")
    assert err < 1e-9
    # l is the rule applied to the kernel's own ssq, up to the device logarithm's last bit
    assert (np.abs(l - G.log_density(q, ssq, 0.5 * data.size, lo, hi)) <= 2 * np.spacing(np.abs(l))).all()


def test_product_coordinates(pkg, gpu_engine, cpu_engine):
    data = _setup(pkg, gpu_engine, cpu_engine)
    x = [np.linspace(4.0, 40.0, 129), np.linspace(0.006, 0.019, 5), np.linspace(0.008, 0.028, 3)]
    l, ssq = (np.asarray(v) for v in gpu_engine.grid_logtarget(x, data, LO3, HI3, "product"))
    q = G.nodes(x, G.PRODUCT)  # NumPy's division
    want = np.asarray(gpu_engine.evidence_logtarget(q, data, LO3, HI3, np.zeros(len(q))))
    assert np.isfinite(l).all() and np.isfinite(want).all()
    ulp = np.abs((l + np.log(q[:, 1])) - want) / np.spacing(np.abs(l))
    print(f"product: l + log x1 against the evidence kernel, {ulp.max():.2f} ulp of |l|")
    assert ulp.max() <= 4.0
    assert np.abs(ssq / _checker_ssq(cpu_engine, data, q) - 1.0).max() < 1e-9


def test_product_window_leaves_the_box(pkg, gpu_engine, cpu_engine):
    """x0 up to 300 with a from 0.005: Dc = x0 / a reaches 60 000, outside [0, 1e4] for whole columns' tails, whole waves among them —
    those nodes are -inf, their ssq NaN, and they are counted per column.  (That a wave wholly outside skips the solve cannot be
    seen from the results: every node outside the box gets the NaN.)"""
    data = _setup(pkg, gpu_engine, cpu_engine)
    x = [np.linspace(4.0, 300.0, 257), np.linspace(0.006, 0.019, 5), np.linspace(0.008, 0.028, 3)]
    w = [G.trapezoid(a) for a in x]
    l, ssq = (np.asarray(v) for v in gpu_engine.grid_logtarget(x, data, LO3, HI3, "product"))
    q = G.nodes(x, G.PRODUCT)
    inb = ((q >= LO3) & (q <= HI3)).all(axis=1)
    assert 0 < (~inb).sum() < len(q) and (~inb).reshape(15, 257)[:, -64:].all()  # whole waves outside
    np.testing.assert_array_equal(np.isfinite(l), inb)
    np.testing.assert_array_equal(np.isnan(ssq), ~inb)
    assert (l[~inb] == -np.inf).all()
    col = gpu_engine.grid_columns(x, w, l, ssq)
    assert col["fields"][:, 5].sum() == (~inb).sum()
    np.testing.assert_array_equal(col["fields"][:, 5], (~inb).reshape(15, 257).sum(axis=1))
    assert np.abs(ssq[inb] / _checker_ssq(cpu_engine, data, q[inb]) - 1.0).max() < 1e-9


def test_product_faces_are_inside(pkg, gpu_engine, cpu_engine):
    """the closed box: nodes on each of the six faces have a density.  Box edges of Dc at powers of two, so that x0 = edge * x1 and
    its division by x1 are exact"""
    data = _setup(pkg, gpu_engine, cpu_engine)
    lo, hi = [512.0, 0.005, 0.005], [8192.0, 0.02, 0.03]
    x1, x2 = np.array([0.005, 0.01, 0.02]), np.array([0.005, 0.02, 0.03])
    x0 = np.array([512.0 * x1[1], 20.0, 40.0, 8192.0 * x1[1]])
    l, _ = (np.asarray(v) for v in gpu_engine.grid_logtarget([x0, x1, x2], data, lo, hi, "product"))
    L = l.reshape(3, 3, 4)  # [i2, i1, i0]
    q = G.nodes([x0, x1, x2], G.PRODUCT).reshape(3, 3, 4, 3)
    assert q[0, 1, 0, 0] == 512.0 and q[0, 1, 3, 0] == 8192.0
    assert np.isfinite(L[:, 1, 0]).all() and np.isfinite(L[:, 1, 3]).all()      # Dc on its lower and upper face
    assert np.isfinite(L[:, 0, 1]).all() and np.isfinite(L[:, 2, 2]).all()      # a = lo, hi (Dc = 4000, 2000 inside)
    assert np.isfinite(L[0, 1, 1:3]).all() and np.isfinite(L[2, 1, 1:3]).all()  # b = lo, hi
    inb = ((q >= lo) & (q <= hi)).all(axis=-1)
    np.testing.assert_array_equal(np.isfinite(L), inb)
    assert (~inb).any()
    # ... and in plain coordinates
    xp = [np.array([512.0, 1000.0, 8192.0]), x1, x2]
    lp, _ = (np.asarray(v) for v in gpu_engine.grid_logtarget(xp, data, lo, hi))
    assert np.isfinite(lp).all()


def _scaled(name, got, want, scale):
    got, want, scale = np.asarray(got, dtype=G.LD), np.asarray(want, dtype=G.LD), np.broadcast_to(np.asarray(scale, dtype=G.LD), np.shape(want))
    err = np.abs(got - want)
    bad = err > TOL * scale + np.finfo(np.float64).tiny  # below float64's normal range a sum is not relatively accurate (long double has the range)
    assert not bad.any(), f"{name}: {int(bad.sum())} entries beyond {TOL} scaled, worst {float((err / np.where(scale > 0, scale, 1)).max()):.2e}"
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


@pytest.mark.parametrize("shape_n,coords", [((257, 9, 7), G.PRODUCT), ((4099, 3, 2), G.PLAIN), ((17, 4), G.PLAIN), ((5,), G.PLAIN)])
def test_reductions_split_path(pkg, gpu_engine, shape_n, coords):
    """crafted l, ssq: a column of all -inf, one -inf node, l spread over 1e4; 4099 nodes per column: 17 rounds of the 256 threads"""
    x, w, center, want, l, ssq = _crafted(shape_n, 11, coords)
    d = len(shape_n)
    got = gpu_engine.grid_columns(x, w, l, ssq, center)
    assert got["lmax"] == want["lmax"]
    f, fw = got["fields"], want["fields"]
    span = np.abs(x[0] - center).max()
    worst = max(_scaled("s0", f[:, 0], fw[:, 0], fw[:, 0]), _scaled("s1", f[:, 1], fw[:, 1], span * fw[:, 0]), _scaled("s2", f[:, 2], fw[:, 2], span ** 2 * fw[:, 0]),
                _scaled("ssq", f[:, 3], fw[:, 3], fw[:, 3]), _scaled("ssq2", f[:, 4], fw[:, 4], fw[:, 4]),
                _scaled("m0", got["m0"], want["m0"], want["m0"]), _scaled("cum0", np.asarray(got["cum0"]), want["cum0"], 1.0))
    np.testing.assert_array_equal(f[:, 5], np.asarray(fw[:, 5], dtype=np.float64))  # the counts are equal
    if d > 1:
        assert not f[1, :5].any() and f[1, 5] == shape_n[0] and not np.asarray(got["cum0"])[1].any()
    lo, hi, shape = [0.5] * d, [10.0] * d, 7.5
    fin, fin_w = gpu_engine.grid_finish(x, w, lo, hi, shape, got["lmax"], f, center, coords), G.finish(x, w, coords, center, shape, lo, hi, want["lmax"], fw)
    q = G.nodes(x, coords)
    sp = q.max(axis=0) - q.min(axis=0)
    worst = max(worst, _scaled("Z", fin["Z"], fin_w["Z"], fin_w["Z"]), _scaled("log_integral", fin["log_integral"], fin_w["log_integral"], abs(fin_w["log_integral"])),
                _scaled("log_evidence", fin["log_evidence"], fin_w["log_evidence"], abs(fin_w["log_evidence"])), _scaled("mean", fin["mean"], fin_w["mean"], sp),
                _scaled("cov", fin["cov"], fin_w["cov"], np.outer(sp, sp)), _scaled("x0_mean", fin["x0_mean"], fin_w["x0_mean"], np.ptp(x[0])),
                _scaled("x0_var", fin["x0_var"], fin_w["x0_var"], np.ptp(x[0]) ** 2), _scaled("std2_mean", fin["std2_mean"], fin_w["std2_mean"], fin_w["std2_mean"]),
                _scaled("std2_var", fin["std2_var"], fin_w["std2_var"], fin_w["std2_mean"] ** 2))
    for k in ("pair", "mass1", "mass2", "cum1", "cum2"):
        worst = max(worst, _scaled(k, fin[k], np.asarray(fin_w[k]).reshape(fin[k].shape), 1.0))
    assert fin["n_neginf"] == fin_w["n_neginf"] == int((l == -np.inf).sum())
    # the CDF of q0 from the library's own tables
    xs = np.linspace(q[:, 0].min() - 0.1, q[:, 0].max() + 0.1, 101)
    F = gpu_engine.grid_cdf(x, got["cum0"], fin["pair"], xs, coords)
    worst = max(worst, _scaled("cdf", F, G.cdf(x, coords, np.asarray(got["cum0"]), fin["pair"], xs), 1.0))
    assert F[0] == 0.0 and abs(F[-1] - 1.0) < TOL and (np.diff(F) >= -TOL).all()
    print(f"{shape_n} coords {coords}: worst scaled error {worst:.2e}")
    # a repeat of the call gives the same bits; host memory gives device memory's bits
    again = gpu_engine.grid_columns(x, w, l, ssq, center)
    with pkg.Engine(mem="device") as dev:
        on_dev = dev.grid_columns(x, w, l, ssq, center)
        F_dev = dev.grid_cdf(x, on_dev["cum0"], fin["pair"], xs, coords)
        on_dev["cum0"] = on_dev["cum0"].cpu().numpy()
    for other in (again, on_dev):
        assert other["lmax"] == got["lmax"]
        for k in ("fields", "m0", "cum0"):
            np.testing.assert_array_equal(np.asarray(other[k]).view(np.int64), np.asarray(got[k]).view(np.int64), err_msg=k)
    np.testing.assert_array_equal(F_dev.view(np.int64), F.view(np.int64))


def test_columns_refuses_nan_and_takes_a_grid_without_density(gpu_engine, pkg):
    x, w = G.simpson(0.0, 1.0, 5)
    with pytest.raises(pkg.RsfError, match="NaN or \\+inf"):
        gpu_engine.grid_columns([x], [w], np.array([0.0, np.nan, 0.0, np.inf, 0.0]), np.ones(5))
    col = gpu_engine.grid_columns([x], [w], np.full(5, -np.inf), np.full(5, np.nan))
    assert col["lmax"] == -np.inf and not col["fields"][:, :5].any() and col["fields"][0, 5] == 5 and not col["m0"].any()
    fin = gpu_engine.grid_finish([x], [w], 0.0, 1.0, 3.0, col["lmax"], col["fields"], col["center"])
    assert fin["log_integral"] == -np.inf and np.isnan(fin["log_evidence"]) and np.isnan(fin["mean"]).all() and fin["n_neginf"] == 5


def _closed_grid(engine, d, n12=65):
    ref, fn, c = R.closed_reference(d)
    if d == 1:
        ax = [G.simpson(c["lo"][0], c["hi"][0], 4001)]
    else:
        ax = [G.simpson(ref.plo, ref.phi, 2001)] + [G.simpson(c["lo"][p], c["hi"][p], n12) for p in (1, 2)]
    post = engine.grid_from_ssq(lambda q: fn(*q.T), [a[0] for a in ax], [a[1] for a in ax], c["lo"], c["hi"], c["shape"], "product" if d == 3 else "plain")
    return post, ref, fn, c


_CLOSED = {}


@pytest.fixture()
def closed(gpu_engine):
    """the closed forms' grid posteriors, tabulated once for the module (host arrays) and served by the test's own engine"""
    def get(d, n12=65):
        if (d, n12) not in _CLOSED:
            _CLOSED[d, n12] = _closed_grid(gpu_engine, d, n12)
        _CLOSED[d, n12][0].engine = gpu_engine
        return _CLOSED[d, n12]
    return get


def test_draws_d2_against_the_specification(gpu_engine):
    """grid_draw_kernel<2, PLAIN>: a crafted (17, 4) grid through the split path, the tables the library's own"""
    x, w, center, _, l, ssq = _crafted((17, 4), 11, G.PLAIN)
    col = gpu_engine.grid_columns(x, w, l, ssq, center)
    fin = gpu_engine.grid_finish(x, w, [0.5] * 2, [10.0] * 2, 7.5, col["lmax"], col["fields"], center)
    q, cell = gpu_engine.grid_draw(x, col["cum0"], fin["cum1"], None, 4096, seed=7, cells=True)
    want = G.draw(x, G.PLAIN, np.asarray(col["cum0"]), fin["cum1"], None, 7, 0, 4096)
    keep = want["margin"] >= 1e-12
    assert (~keep).sum() <= 2
    np.testing.assert_array_equal(cell[keep], want["cell"][keep])
    assert (np.abs(np.asarray(q)[keep] - want["q"][keep]) <= 4 * np.spacing(np.abs(want["q"][keep]))).all()
    assert (np.unique(cell[:, 1]).size > 1) and not (want["cell"][keep][:, 1] == 1).all()
    assert fin["pair"][0, 1] == 0.0  # a column without mass: draws conditioned on it take the rule's x[k] of an empty cell, as the specification's do


@pytest.mark.parametrize("d", [1, 3])
def test_draws_against_the_specification(gpu_engine, closed, d):
    """4096 draws, two shards of one stream; from the library's own tables the specification's inversion finds the same cells and
    x within 4 ulp.  Draws whose u lies within 1e-12 of a table entry are left out: at most 2 of 4096 (about 1e-5 expected)"""
    post, _, _, _ = closed(d, 33)
    tables = (post.x, post.cum0, post.finish["cum1"], post.finish["cum2"])
    q, cell = gpu_engine.grid_draw(*tables, 4096, post.coords, seed=5, offset=0, cells=True)
    q2, cell2 = gpu_engine.grid_draw(*tables, 3096, post.coords, seed=5, offset=1000, cells=True)
    np.testing.assert_array_equal(np.asarray(q)[1000:].view(np.int64), np.asarray(q2).view(np.int64))
    np.testing.assert_array_equal(cell[1000:], cell2)
    want = G.draw(post.x, post.coords, np.asarray(post.cum0), post.finish["cum1"], post.finish["cum2"], 5, 0, 4096)
    keep = want["margin"] >= 1e-12
    assert (~keep).sum() <= 2
    np.testing.assert_array_equal(cell[keep], want["cell"][keep])
    ulp = np.abs(np.asarray(q)[keep] - want["q"][keep]) / np.spacing(np.abs(want["q"][keep]))
    print(f"d = {d}: {int((~keep).sum())} draws left out, x within {ulp.max():.2f} ulp")
    assert ulp.max() <= 4.0
    lo, hi = np.asarray(post.lo), np.asarray(post.hi)
    assert ((np.asarray(q) >= lo) & (np.asarray(q) <= hi)).all()


def _closed_draws(post, ref, tag, seed):
    q, std2 = post.draw(N_DRAWS, seed=seed)
    fails = []
    zmax, kmax = R.check(tag, ref, q, std2, fails)
    print(f"{tag}: largest |z| {zmax:.2f}, largest sqrt(C) D {kmax:.2f}")
    return fails, zmax


def test_closed_form_d1(closed):
    post, ref, _, c = closed(1)
    import evidence_cases
    err = post.log_integral - evidence_cases.CLOSED_TRUTH[1]
    print(f"d = 1: log I - truth {err:+.2e}")
    assert abs(err) < 1e-10 and post.n_neginf == 0
    fails, _ = _closed_draws(post, ref, "closed d = 1", 1)
    assert not fails, fails
    mg = ref.marg["Dc"]
    assert abs(post.mean[0] - mg.mean) < 1e-9 * mg.sd and abs(post.cov[0, 0] / mg.var - 1.0) < 1e-9
    shift = np.abs(post.quantiles("Dc", R.PROBS) - mg.quantiles()) / R.se_table(ref, N_DRAWS)["Dc"]["q"]
    print(f"Dc quantiles against the reference: {shift.max():.2e} SE")
    assert shift.max() < 0.25


@pytest.mark.parametrize("seed", [1, 2])
def test_closed_form_d3(closed, seed):
    """(2001, 65, 65) in product coordinates on the reference's window: 8.5 M nodes through the reductions"""
    post, ref, _, _ = closed(3)
    fails, _ = _closed_draws(post, ref, f"closed d = 3 seed {seed}", seed)
    assert not fails, fails
    for k, name in enumerate(("Dc", "a", "b")):
        mg = ref.marg[name]
        assert abs(post.mean[k] - mg.mean) < 1e-5 * mg.sd and abs(post.cov[k, k] / mg.var - 1.0) < 2e-5, name
    assert abs(post.std2_mean - ref.marg["sigma2"].mean) < 1e-5 * ref.marg["sigma2"].sd
    # Dc's CDF where Dc is not an axis: against the reference's quantiles, in the reference's Monte-Carlo SE at C = 262 144
    se = R.se_table(ref, N_DRAWS)["Dc"]["q"]
    shift = np.abs(post.quantiles("Dc", R.PROBS) - ref.marg["Dc"].quantiles()) / se
    print(f"Dc quantiles against the reference: {shift.max():.3f} SE")
    assert shift.max() < 0.25


def test_closed_form_d3_33_nodes_show_the_trapezoid_cdf(closed):
    post, ref, _, _ = closed(3, 33)
    fails, zmax = _closed_draws(post, ref, "closed d = 3, 33 nodes", 1)
    assert fails and zmax > R.Z_MAX


def test_real_model_d1(pkg, gpu_engine, cpu_engine):
    """Posterior1's own fine nodes and Simpson weights: the same quadrature rule, so the distance is the solves' alone"""
    ref, data = _reference(pkg, cpu_engine, 1, *BOX1)
    gpu_engine.set_model(_model(pkg), 1)
    shape = ref.shape
    x, w = ref.x, R._simpson_weights(ref.x)
    l, ssq = gpu_engine.grid_logtarget([x], data, *BOX1)
    col = gpu_engine.grid_columns([x], [w], l, ssq)
    fin = gpu_engine.grid_finish([x], [w], BOX1[0], BOX1[1], shape, col["lmax"], col["fields"], col["center"])
    mg = ref.marg["Dc"]
    e_logi = fin["log_integral"] - (np.log(ref.Z) + ref.lmax)
    e_mean, e_var = (fin["mean"][0] - mg.mean) / mg.sd, fin["cov"][0, 0] / mg.var - 1.0
    print(f"real d = 1: log I {e_logi:+.2e} (bound {shape * 1e-9:.1e}), mean {e_mean:+.2e} SD, variance {e_var:+.2e} relative (bound {4 * shape * 1e-9:.1e})")
    assert abs(e_logi) < shape * 1e-9 and abs(e_mean) < 4 * shape * 1e-9 and abs(e_var) < 4 * shape * 1e-9
    s2 = ref.marg["sigma2"]
    assert abs(fin["std2_mean"] / s2.mean - 1.0) < 4 * shape * 1e-9 and abs(fin["std2_var"] / s2.var - 1.0) < 4 * shape * 1e-9
    # Engine.grid_posterior with its own window
    post = gpu_engine.grid_posterior(data, *BOX1)
    print(f"grid_posterior: window [{post.x[0][0]:.3f}, {post.x[0][-1]:.3f}] (reference [{ref.wlo:.3f}, {ref.whi:.3f}]), outside {post.outside:.2e}")
    assert post.outside < 1e-9 and post.n == (4001,) and post.n_neginf == 0
    assert abs(post.log_integral - (np.log(ref.Z) + ref.lmax)) < 1e-6 and abs(post.mean[0] - mg.mean) < 1e-6 * mg.sd
    fails = []
    R.check("real d = 1 draws", ref, *post.draw(N_DRAWS, seed=3), fails)
    assert not fails, fails


def test_real_model_d3_against_the_reference_quadrature(pkg, gpu_engine, cpu_engine):
    """Engine.grid_posterior at its defaults against Posterior3 at its own.  Nothing here can be derived — the reference
    interpolates log SSq by a spline — so the yardstick is the reference's own resolution distance: grid_shift_in_se between
    Posterior3 at its defaults and at (n_ab 48, n_pc 193), C = 262 144, recorded by tools/grid_self_distance.py in
    tests/golden/grid_self_distance.json.  Per quantity the GPU-to-reference shift stays below 8 x that (the margin DESIGN 4d
    uses), or below 0.25 SE where the self-distance is smaller.

    Measured on the MI355X: every mean, variance and quantile of Dc, a, b, Dc a and sigma^2 within 0.009 SE.  Dc's quantiles come
    from GridPosterior.dc_cdf, which takes rsf_grid_cdf's sum on the a axis refined four times: on the grid's own 65 a nodes the
    0.975 quantile was 0.322 SE off (with 129 a nodes solved 0.013, with 257 0.000; more b nodes or CDF points changed nothing) —
    F0(x a | a, b) is a step in a about one node spacing wide at the face a = lo, where Dc's upper tail lies."""
    ref, data = _reference(pkg, cpu_engine, 3, LO3, HI3)
    with open(os.path.join(GOLDEN, "grid_self_distance.json")) as f:
        rec = json.load(f)
    assert rec["C"] == N_DRAWS and rec["box"] == [LO3, HI3]
    gpu_engine.set_model(_model(pkg), 1)
    post = gpu_engine.grid_posterior(data, LO3, HI3)
    assert post.n == (2001, 65, 65) and post.coords == G.PRODUCT and post.outside < 1e-9
    se = R.se_table(ref, N_DRAWS)
    got = {"Dc": (post.mean[0], post.cov[0, 0]), "a": (post.mean[1], post.cov[1, 1]), "b": (post.mean[2], post.cov[2, 2]),
           "Dc*a": (post.x0_mean, post.x0_var), "sigma2": (post.std2_mean, post.std2_var)}
    fails = []
    for name, (m, v) in got.items():
        mg = ref.marg[name]
        s = [abs(m - mg.mean) / se[name]["mean"], abs(v - mg.var) / se[name]["var"]]
        if name != "sigma2":
            s += list(np.abs(post.quantiles(name, R.PROBS) - mg.quantiles()) / se[name]["q"])
        bound = max(8.0 * rec["shift_in_se"][name], 0.25)
        print(f"real d = 3 {name}: shift {max(s):.3f} SE (the reference's own {rec['shift_in_se'][name]:.3f}, bound {bound:.3f}); mean, variance, quantiles: "
              + " ".join(f"{v:.3f}" for v in s))
        if not max(s) < bound:
            fails.append(f"{name}: {max(s):.3f} SE >= {bound:.3f}")
    assert not fails, fails
    R.check("real d = 3 draws", ref, *post.draw(N_DRAWS, seed=4), fails)
    assert not fails, fails


def test_cross_checks(pkg, gpu_engine, cpu_engine):
    """log_evidence against bridge sampling on the grid's own draws (within 4.5 re); MCMC.quadrature's pool feeds predictive and
    rank_diagnostics unchanged"""
    ref, data = _reference(pkg, cpu_engine, 1, *BOX1)
    model = _model(pkg)
    mc = pkg.MCMC(model, data, 1000.0, ["Uniform", BOX1[0], BOX1[1]], 1000.0, nsamples=10, verbose=False)
    post = mc.quadrature(n_draws=1024, mem="host")
    try:
        assert post.q.shape == (1024, 1) and post.std2.shape == (1024,) and np.isfinite(post.std2).all()
        pool = post.pool(16384, seed=9)
        assert pool.samples.shape == (16, 1024, 1) and pool.stats["log_evidence"] == post.log_evidence
        ev = post.engine.evidence(pool.samples.reshape(-1, 1), data, [BOX1[0]], [BOX1[1]], seed=2, ess_factor=1.0)
        z = (ev["log_evidence"] - post.log_evidence) / ev["re"]
        print(f"log evidence: grid {post.log_evidence:.6f}, bridge {ev['log_evidence']:.6f} +- {ev['re']:.2e} (z {z:+.2f})")
        assert abs(z) < R.Z_MAX
        pred = pool.predictive(model, data, engine=post.engine)
        assert np.isfinite(pred["elpd_waic"]) and abs(pred["mean_std2"] / post.std2_mean - 1.0) < R.Z_MAX * np.sqrt(post.std2_var / 16384) / post.std2_mean
        rd = pool.rank_diagnostics(engine=post.engine)[0]
        assert rd["rhat"] < 1.01 and rd["ess_bulk"] > 0.8 * 16384  # independent draws
        np.testing.assert_allclose(rd["median"], post.quantiles("Dc", [0.5])[0], atol=R.Z_MAX * ref.marg["Dc"].sd * 1.2533 / np.sqrt(16384))
    finally:
        post.engine.close()


def _code(pkg, call):
    try:
        call()
    except pkg.RsfError as e:
        return e.code
    return 0


def test_error_invalid_arguments(pkg):
    """the ctx entry points' own checks, through the Engine and through C"""
    abi = pkg._abi
    ip = lambda v: np.array(v, dtype=np.int32).ctypes.data_as(abi._I32P)
    dp = lambda v: np.array(v, dtype=np.float64).ctypes.data_as(abi._DP)
    P = lambda a: a.ctypes.data
    x3 = [np.linspace(4.0, 40.0, 5), np.linspace(0.006, 0.019, 3), np.linspace(0.008, 0.028, 3)]
    data = np.cos(np.linspace(0.0, 3.0, 500))
    with pkg.Engine(mem="host") as eng:
        x1 = [np.linspace(500.0, 1500.0, 5)]
        assert _code(pkg, lambda: eng.lib and abi.check(eng.lib, eng.lib.rsf_grid_logtarget(eng._ctx, 1, ip([5]), dp(x1[0]), P(data), 250.0, dp([0.0]), dp([1e4]), 0,
                                                                                           P(np.empty(5)), P(np.empty(5))))) == -3  # no model
        eng.set_model(_model(pkg), 1)
        assert np.isfinite(np.asarray(eng.grid_logtarget(x3, data, LO3, HI3, "product")[0])).all()
        for kw in (dict(shape=0.0), dict(shape=np.nan), dict(lo=[0.0, 0.0, 0.005]), dict(lo=[0.0, -1.0, 0.005]), dict(hi=[1e4, 0.005, 0.03]), dict(hi=[np.inf, 0.02, 0.03])):
            args = dict(x=x3, data=data, lo=LO3, hi=HI3, coords="product", shape=250.0)
            args.update(kw)
            assert _code(pkg, lambda: eng.grid_logtarget(**args)) == -1, kw
        for x in ([x3[0][::-1].copy(), x3[1], x3[2]], [x3[0], np.array([0.01]), x3[2]], [x3[0], np.array([0.01, np.nan, 0.02]), x3[2]]):
            assert _code(pkg, lambda: eng.grid_logtarget(x, data, LO3, HI3)) == -1
        lib, ctx, l, q = eng.lib, eng._ctx, np.empty(45), np.empty(45)
        ok = [ctx, 3, ip([5, 3, 3]), dp(np.concatenate(x3)), P(data), 250.0, dp(LO3), dp(HI3), 1, P(l), P(q)]
        assert lib.rsf_grid_logtarget(*ok) == 0
        for i, v in ((0, None), (1, 2), (1, 4), (2, None), (3, None), (4, None), (6, None), (7, None), (8, 2), (8, -1), (9, None), (10, None)):
            bad = list(ok)
            bad[i] = v
            assert lib.rsf_grid_logtarget(*bad) == -1, i
        assert lib.rsf_grid_logtarget(ctx, 1, ip([5]), dp(x1[0]), P(data), 250.0, dp([0.0]), dp([1e4]), 1, P(l), P(q)) == -1  # PRODUCT needs d = 3
    # the split calls: d = 1..3, no model needed
    with pkg.Engine(mem="host") as bare:
        x, w, center, _, l, ssq = _crafted((17, 4), 11, G.PLAIN)
        col = bare.grid_columns(x, w, l, ssq, center)
        fin = bare.grid_finish(x, w, [0.5] * 2, [10.0] * 2, 7.5, col["lmax"], col["fields"], center)
        assert _code(pkg, lambda: bare.grid_columns(x, w, l, ssq, np.inf)) == -1
        assert _code(pkg, lambda: bare.grid_columns(x, [w[0], -w[1]], l, ssq)) == -1
        assert _code(pkg, lambda: bare.grid_columns([x[0], x[1][::-1].copy()], w, l, ssq)) == -1
        for kw in (dict(n=0), dict(n=-3), dict(offset=-1)):
            args = dict(n=8, seed=1, offset=0)
            args.update(kw)
            assert _code(pkg, lambda: bare.grid_draw(x, col["cum0"], fin["cum1"], None, **args)) == -1, kw
        assert _code(pkg, lambda: bare.grid_cdf(x, col["cum0"], fin["pair"], np.empty(0))) == -1  # nx < 1
        lib, ctx, n, xc = bare.lib, bare._ctx, ip([17, 4]), dp(np.concatenate(x))
        out = np.empty((8, 2))
        assert lib.rsf_grid_draw(ctx, 2, n, xc, 0, P(col["cum0"]), dp(fin["cum1"]), None, 1, 0, 8, P(out), None) == 0
        assert lib.rsf_grid_draw(ctx, 2, n, xc, 0, P(col["cum0"]), None, None, 1, 0, 8, P(out), None) == -1       # cum1 is needed at d = 2
        assert lib.rsf_grid_draw(ctx, 2, n, xc, 1, P(col["cum0"]), dp(fin["cum1"]), None, 1, 0, 8, P(out), None) == -1  # PRODUCT needs d = 3
        assert lib.rsf_grid_draw(ctx, 2, n, xc, 0, None, dp(fin["cum1"]), None, 1, 0, 8, P(out), None) == -1
        assert lib.rsf_grid_draw(None, 2, n, xc, 0, P(col["cum0"]), dp(fin["cum1"]), None, 1, 0, 8, P(out), None) == -1
        assert lib.rsf_grid_cdf(ctx, 2, n, xc, 2, P(col["cum0"]), dp(fin["pair"]), 1, dp([1.5]), dp([0.0])) == -1
        assert lib.rsf_grid_cdf(ctx, 2, n, xc, 0, P(col["cum0"]), None, 1, dp([1.5]), dp([0.0])) == -1
        assert b"NULL" in lib.rsf_last_error()
        assert lib.rsf_grid_columns(ctx, 2, n, xc, None, P(l), P(ssq), center, dp([0.0]), P(np.empty((4, 6))), None, None) == -1


def test_error_unsupported_integrator_and_the_float32_model(pkg):
    x = [np.linspace(300.0, 3000.0, 129)]
    data = np.cos(np.linspace(0.0, 3.0, 500))
    with pkg.Engine(mem="host") as eng:
        m = _model(pkg)
        m.integrator = "dop853"
        eng.set_model(m, 1)
        assert _code(pkg, lambda: eng.grid_logtarget(x, data, *BOX1)) == -5
        # a float32 model gets the float64 solve: the bits of the float64 model
        m = _model(pkg)
        m.precision = "float32"
        eng.set_model(m, 1)
        a = [np.asarray(v) for v in eng.grid_logtarget(x, data, *BOX1)]
        eng.set_model(_model(pkg), 1)
        b = [np.asarray(v) for v in eng.grid_logtarget(x, data, *BOX1)]
        for u, v in zip(a, b):
            assert np.isfinite(u).all()
            np.testing.assert_array_equal(u.view(np.int64), v.view(np.int64))
