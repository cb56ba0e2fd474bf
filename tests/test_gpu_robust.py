"""Robust losses on the device (mvba_create_robust, mvba_residuals) against the NumPy reference of
tests/_robust_ref.py: the reduced system and the step in every Schur form, trajectories, recovery from gross outliers,
the squared limit, sharding, the accessors and a config-3-sized run."""
import numpy as np
import pytest

from _robust_ref import RobustOracleEngine, inject_outliers, rho, robust_cost, weight
from lib.bundle_adjustment import BundleAdjuster, dense_to_observations, lm_loop, to_gauge_frame
from lib.synthetic import make_scene
from oracle import ba_oracle as O

pytestmark = pytest.mark.gpu


def _close(a, b, tol, what=""):
    scale = max(np.abs(b).max(), 1e-300)
    err = np.abs(np.asarray(a) - np.asarray(b)).max()
    assert err <= tol * scale, (what, err, scale)


def _problem(sc, xy):
    X, R, t = to_gauge_frame(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    return (sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, xy, 1.0, sc.axis, X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)


def _engines(prob, loss, scale):
    from lib._mvba import HipEngine

    n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R = prob
    eng = HipEngine(n, m, pt_ptr, cam, xy, f0, axis, loss=loss, loss_scale=scale)
    eng.set_params(X, f, u, t, R)
    g = RobustOracleEngine(n, m, pt_ptr, cam, xy, f0, axis, loss=loss, loss_scale=scale)
    g.set_params(X, f, u, t, R)
    return eng, g


def _check_step(eng, g, c=1e-3, tol=1e-10):
    """Cost, the weighted rows, A_full / b_full, the trial state and the trial cost against the reference."""
    _close(eng.cost(), g.cost(), 1e-12, "cost")
    eng.linearize()
    g.linearize()
    n_obs = g.xy.shape[0]
    _close(eng.debug_read("weight") ** 2, g.w, 1e-12, "weight")
    _close(eng.debug_read("residual").reshape(n_obs, 2), g.e, 1e-11, "residual")
    _close(eng.debug_read("JX").reshape(n_obs, 2, 3), g.JX, 1e-11, "JX")
    _close(eng.debug_read("JC").reshape(n_obs, 2, 9), g.JC, 1e-11, "JC")
    E1 = eng.try_step(c)
    A, b = g.reduced_system(c)
    E1o = g.try_step(c)
    m9 = 9 * g.m
    _close(eng.debug_read("A_full").reshape(m9, m9), A, tol, "A_full")
    _close(eng.debug_read("b_full"), b, tol, "b_full")
    _close(eng.debug_read("dX").reshape(-1, 3), g.dX, 1e-9, "dX")
    _close(eng.debug_read("trial_X").reshape(-1, 3), g.tX, tol, "trial_X")
    tc = eng.debug_read("trial_cam").reshape(g.m, 15)
    _close(tc[:, 0], g.tf, tol, "trial f")
    _close(tc[:, 3:6], g.tt, 1e-9, "trial t")
    # (the trial cost sums rho over a state that agrees to ~1e-9 (dX): Huber's 2 sqrt(b s) of the outliers carries that to
    # 1e-10 .. 4e-10 relative -- measured; the squared parity tests hold the trial cost to 1e-9 too)
    assert E1 == pytest.approx(E1o, rel=1e-9)
    return E1


def _scene(n, m, p, frac=0.08, seed=5):
    sc = make_scene(n, m, vis_p=p)
    xy, mask = inject_outliers(sc.xy, frac, 20.0, 100.0, seed=seed)
    return sc, xy, mask


FORMS = [  # (points, cameras, visibility, MVBA_SCHUR, MVBA_FORCE_BIG, expected form)
    (1500, 12, 0.4, "pairs", None, "pairs"),
    (300, 10, 1.0, "dense", None, "dense"),
    (400, 14, 0.8, "dense", None, "dense"),    # missing observations: the table form
    (900, 9, 0.5, "pairs", "1", "pairs"),      # the 64-bit-offset kernel
    (3000, 647, 0.04, None, None, "pairs"),    # GCAM: camera tables in device memory
]


@pytest.mark.parametrize("loss,scale", [("huber", 3.0), ("cauchy", 2.0)])
@pytest.mark.parametrize("n,m,p,schur,big,form", FORMS)
def test_reduced_system_and_step_match_the_reference(monkeypatch, loss, scale, n, m, p, schur, big, form):
    if schur:
        monkeypatch.setenv("MVBA_SCHUR", schur)
    if big:
        monkeypatch.setenv("MVBA_FORCE_BIG", big)
    sc, xy, _ = _scene(n, m, p)
    eng, g = _engines(_problem(sc, xy), loss, scale)
    assert eng.schur_info()["kernel"] == form
    _check_step(eng, g)
    assert g.w.min() < 0.5  # the outliers are down-weighted


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_slot_form_request_runs_the_unit_form(monkeypatch, loss):
    monkeypatch.setenv("MVBA_SCHUR", "slots")
    sc, xy, _ = _scene(4000, 40, 0.3)
    eng, g = _engines(_problem(sc, xy), loss, 2.5)
    assert eng.schur_info()["kernel"] == "pairs"
    _check_step(eng, g)


@pytest.mark.parametrize("name,axis,args", [("linearize_60x7_xright", "x-right_z-forward", (10.0, 1e-8, 8)),
                                             ("visibility_300x12", "x-up_z-forward", (2.0, -1.0, 10))])
@pytest.mark.parametrize("loss,scale", [("huber", 2.0), ("cauchy", 1.0)])
def test_trajectory_matches_the_reference_lm_loop(golden, name, axis, args, loss, scale):
    d = golden(name)
    vis = d["vis"] if "vis" in d.files else None
    x = np.array(d["x"], np.float64, copy=True)
    live = np.argwhere(vis) if vis is not None else np.argwhere(np.ones(x.shape[:2], bool))
    rng = np.random.default_rng(11)
    pick = live[rng.choice(len(live), size=max(1, len(live) // 15), replace=False)]
    ang = rng.uniform(0, 2 * np.pi, len(pick))
    r = rng.uniform(20.0, 100.0, len(pick))
    x[pick[:, 0], pick[:, 1]] += np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    ba = BundleAdjuster(x, d["init_X"], d["init_K"], d["init_R"], d["init_t"], visibility_index=vis, axis=axis, loss=loss,
                        loss_scale=scale)
    ba.optimize(*args, is_debug=True)
    log = ba.get_log()
    n, m = x.shape[:2]
    pt_ptr, cam, xy = dense_to_observations(x, vis)
    g = RobustOracleEngine(n, m, pt_ptr, cam, xy, 1.0, axis, loss=loss, loss_scale=scale)
    X, R, t = O.normalize_scene(d["init_X"], d["init_R"], d["init_t"], axis)
    g.set_params(X, d["init_K"][:, 0, 0], d["init_K"][:, :2, 2], t, R)
    states, Es = [], []

    def on_state(E):
        states.append(tuple(v.copy() for v in g.get_params()))
        Es.append(E)

    lm_loop(g, *args, on_state=on_state, verbose=False)
    E = np.array([e["reprojection_error"] for e in log])
    assert len(E) == len(Es)
    assert ba._engine.n_solves == g.n_solves
    np.testing.assert_allclose(E, Es, rtol=1e-9, atol=1e-12)
    Xg, _, _, tg, Rg = states[-1]
    np.testing.assert_allclose(log[-1]["points"], Xg, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(log[-1]["pos"], tg, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(log[-1]["basis"], Rg, rtol=1e-9, atol=1e-9)


def _aligned_errors(X, t, X_gt, t_gt):
    """RMS point and camera-position error after the best similarity onto the ground truth (gauge-free)."""
    mu, mg = X.mean(0), X_gt.mean(0)
    A, B = X - mu, X_gt - mg
    U, S, Vt = np.linalg.svd(B.T @ A)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    Q = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / (A * A).sum()
    f = lambda P: s * (P - mu) @ Q.T + mg
    return np.sqrt(((f(X) - X_gt) ** 2).sum(1).mean()), np.sqrt(((f(t) - t_gt) ** 2).sum(1).mean())


def test_robust_losses_recover_from_gross_outliers():
    sc = make_scene(800, 10, vis_p=0.7)
    # make_scene's images have f ~ 1 and noise 1e-3 (1 px at f = 1000): the outliers are 20-100 px, i.e. 0.02-0.1 units.  (With
    # displacements of 30-100 units -- a hundred image widths -- Huber's unbounded influence drags the cameras off while Cauchy
    # still recovers: measured, and why the scales below are a few times the noise.)
    xy_bad, mask = inject_outliers(sc.xy, 0.10, 0.02, 0.1, seed=9)
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    inl = np.ones(sc.n_points, bool)
    inl[np.unique(pt[mask])] = False

    def fit(xy, **kw):
        ba = BundleAdjuster.from_observations(sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, xy, sc.init_X, sc.init_K,
                                              sc.init_R, sc.init_t, axis=sc.axis, **kw)
        X, K, R, t = ba.optimize(2.0, -1.0, 60)
        return _aligned_errors(X[inl], t, sc.X_gt[inl], sc.t_gt), ba

    (clean_X, clean_t), _ = fit(sc.xy)
    (sq_X, sq_t), _ = fit(xy_bad)
    # measured (aligned RMS error of inlier points / camera positions): clean squared 0.0041 / 0.014, squared with the outliers
    # 0.013 / 0.256, Huber 0.0043 / 0.032, Cauchy 0.0042 / 0.015
    for loss, scale in (("huber", 0.003), ("cauchy", 0.003)):
        (rX, rt), ba = fit(xy_bad, loss=loss, loss_scale=scale)
        assert rX <= 3.0 * clean_X and rt <= 3.0 * clean_t, (loss, rX, rt, clean_X, clean_t)
        w = ba.weights()
        assert np.median(w[mask]) < 0.2 and np.median(w[~mask]) > 0.9  # the outliers are the ones discounted
    assert sq_X > 3.0 * clean_X or sq_t > 3.0 * clean_t, (sq_X, sq_t, clean_X, clean_t)


def test_squared_through_create_robust_is_bitwise_the_plain_engine():
    from lib._mvba import HipEngine

    sc, xy, _ = _scene(1200, 12, 0.5)
    n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R = _problem(sc, xy)
    runs = []
    for kw in ({}, {"loss": "squared", "loss_scale": 5.0}):
        eng = HipEngine(n, m, pt_ptr, cam, xy, f0, axis, **kw)
        eng.set_params(X, f, u, t, R)
        E = lm_loop(eng, 2.0, -1.0, 6, verbose=False)
        runs.append((E, eng.n_solves, eng.get_params()))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for a, b in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("schur", ["pairs", "dense"])
def test_huber_above_every_residual_matches_the_squared_engine(monkeypatch, schur):
    from lib._mvba import HipEngine

    monkeypatch.setenv("MVBA_SCHUR", schur)
    sc = make_scene(400, 8, vis_p=1.0 if schur == "dense" else 0.6)
    n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R = _problem(sc, sc.xy)
    big = 1e3 * (1.0 + np.abs(O.residuals(X, f, u, t, R, 1.0, np.repeat(np.arange(n), np.diff(pt_ptr)), cam, xy)).max())
    out = []
    for kw in ({}, {"loss": "huber", "loss_scale": big}):
        eng = HipEngine(n, m, pt_ptr, cam, xy, f0, axis, **kw)
        eng.set_params(X, f, u, t, R)
        E = lm_loop(eng, 2.0, -1.0, 5, verbose=False)
        out.append((E, eng.n_solves, eng.get_params()))
    # (w = 1 exactly on every row, but the robust instantiations are compiled code of their own: contraction into FMAs
    # differs, 5e-12 relative after five iterations -- measured)
    assert out[0][1] == out[1][1]
    assert out[1][0] == pytest.approx(out[0][0], rel=1e-12)
    for a, b in zip(out[0][2], out[1][2]):
        _close(b, a, 1e-10)


def test_two_thread_ranks_host_transport():
    from lib import _distributed as D
    from lib._mvba import HipEngine

    sc, xy_bad, _ = _scene(3000, 20, 0.3)
    n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R = _problem(sc, xy_bad)
    one = HipEngine(n, m, pt_ptr, cam, xy, f0, axis, loss="huber", loss_scale=2.0)
    one.set_params(X, f, u, t, R)
    E_one = [one.cost()]
    lm_loop(one, 2.0, -1.0, 4, on_state=E_one.append, verbose=False)
    parts = D.partition_points(pt_ptr, 2)

    def body(rank, g):
        lo, hi = parts[rank]
        p2, c2, x2 = D.slice_observations(pt_ptr, cam, xy, lo, hi)
        eng = HipEngine(hi - lo, m, p2, c2, x2, f0, axis, loss="huber", loss_scale=2.0)
        g.attach(eng, rank)
        eng.set_params(X[lo:hi], f, u, t, R)
        Es = [eng.cost()]
        lm_loop(eng, 2.0, -1.0, 4, on_state=Es.append, verbose=False)
        return Es, eng.get_params(), eng.residuals()

    res = D.InProcessGroup(2).run(body)
    for r in res:
        np.testing.assert_allclose(r[0], E_one, rtol=1e-12)
    for i in (1, 2, 3, 4):  # cameras: bitwise equal on both ranks
        assert np.array_equal(res[0][1][i], res[1][1][i])
    _close(res[0][1][1], one.get_params()[1], 1e-9, "f")
    e_one = one.residuals()
    lo, hi = parts[1]
    assert res[1][2].shape == (pt_ptr[hi] - pt_ptr[lo], 2)
    _close(np.concatenate([res[0][2], res[1][2]]), e_one, 1e-7, "residuals")


def test_accessors_and_reproducibility():
    sc, xy, mask = _scene(2000, 16, 0.4)
    kw = dict(axis=sc.axis, loss="cauchy", loss_scale=3.0)
    runs = []
    for _ in range(2):
        ba = BundleAdjuster.from_observations(sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, xy, sc.init_X, sc.init_K,
                                              sc.init_R, sc.init_t, **kw)
        runs.append((ba.optimize(2.0, -1.0, 6), ba))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)
    ba = runs[0][1]
    X, K, R, t = runs[0][0]
    e = ba.residuals()
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    # projection of the returned (input-frame) estimate minus the observations
    Xc = np.einsum("oji,oj->oi", R[sc.cam_idx], X[pt] - t[sc.cam_idx])
    p = np.einsum("oij,oj->oi", K[sc.cam_idx], Xc)
    ref = p[:, :2] / p[:, 2:3] - xy
    _close(e, ref, 1e-12, "residuals")
    w = ba.weights()
    np.testing.assert_allclose(w, 1.0 / (1.0 + (e * e).sum(1) / 9.0), rtol=1e-14)
    with pytest.raises(NotImplementedError):
        ba.covariance()
    with pytest.raises(ValueError):
        ba._engine.covariance()


def test_dense_constructor_residual_order_and_weights():
    sc = make_scene(200, 6, vis_p=1.0)
    x, vis = sc.dense()
    ba = BundleAdjuster(x, sc.init_X, sc.init_K, sc.init_R, sc.init_t, visibility_index=vis, axis=sc.axis, loss="huber",
                        loss_scale=1.0)
    e = ba.residuals()
    pt_ptr, cam, xy = dense_to_observations(x, vis)
    assert e.shape == (len(cam), 2)
    assert np.array_equal(ba.weights() <= 1.0, np.ones(len(cam), bool))


def test_config3_huber_five_iterations():
    from lib._mvba import HipEngine

    sc = make_scene(1_000_000, 100, vis_p=0.1)
    n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R = _problem(sc, sc.xy)
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    e0 = O.residuals(X, f, u, t, R, 1.0, pt, cam, xy)
    delta = float(np.median(np.sqrt((e0 * e0).sum(1))))  # half the observations on Huber's linear branch
    eng = HipEngine(n, m, pt_ptr, cam, xy, f0, axis, loss="huber", loss_scale=delta)
    eng.set_params(X, f, u, t, R)
    Es = [eng.cost()]
    lm_loop(eng, 10.0, -1.0, 5, on_state=Es.append, verbose=False)
    assert all(b <= a for a, b in zip(Es, Es[1:])), Es
    X1, f1, u1, t1, R1 = eng.get_params()
    E_np = robust_cost(X1, f1, u1, t1, R1, 1.0, pt, cam, xy, delta * delta, "huber")
    assert eng.cost() == pytest.approx(E_np, rel=1e-12)
