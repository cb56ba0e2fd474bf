"""Marginal covariances on the device (mvba_covariance / HipEngine.covariance / BundleAdjuster.covariance) against the NumPy
references of tests/_covariance_ref.py, in every Schur form, sharded, and at config-3 size."""
import numpy as np
import pytest

from _covariance_ref import point_blocks, schur_covariance
from lib.bundle_adjustment import (BundleAdjuster, LevenbergMarquardt, covariance_to_input_frame, dense_to_observations,
                                   lm_loop, to_gauge_frame)
from lib.synthetic import make_scene

pytestmark = pytest.mark.gpu


def _close(a, b, tol, what=""):
    scale = np.abs(b).max()
    err = np.abs(a - b).max()
    assert err <= tol * scale, (what, err, scale)


def _problem_from_scene(sc):
    X, R, t = to_gauge_frame(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    return (sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis, X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2],
            t, R)


def _problem_from_golden(golden, name, axis):
    d = golden(name)
    x = d["x"]
    pt_ptr, cam, xy = dense_to_observations(x, d["vis"] if "vis" in d.files else None)
    xy = np.ascontiguousarray(xy.transpose(1, 0, 2).reshape(-1, 2)) if xy.ndim == 3 else xy  # (image planes -> obs order)
    X, R, t = to_gauge_frame(d["init_X"], d["init_R"], d["init_t"], axis)
    return (x.shape[0], x.shape[1], pt_ptr, cam, xy, 1.0, axis, X, d["init_K"][:, 0, 0], d["init_K"][:, :2, 2], t, R)


def _engine(prob):
    from lib._mvba import HipEngine

    n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R = prob
    eng = HipEngine(n, m, pt_ptr, cam, xy, f0, axis)
    eng.set_params(X, f, u, t, R)
    return eng


def _check(prob, tol=1e-8):
    got = _engine(prob).covariance(full=True)
    ref = schur_covariance(*prob)
    _close(got["points"], ref["points"], tol, "points")
    _close(got["cameras"], ref["cameras"], tol, "cameras")
    _close(got["cameras_full"], ref["cameras_full"], tol, "cameras_full")
    return got


@pytest.mark.parametrize("name,axis", [("euclid_default", "x-up_z-forward"), ("visibility_300x12", "x-right_z-forward")])
def test_golden_scenes_match_the_reference(golden, name, axis):
    _check(_problem_from_golden(golden, name, axis))


@pytest.mark.parametrize("n,m,p", [(2000, 12, 0.4), (777, 33, 0.15), (90, 70, 1.0)])  # last: 70 observations per point > 64
def test_random_scenes_match_the_reference(n, m, p):
    got = _check(_problem_from_scene(make_scene(n, m, vis_p=p)))
    assert np.array_equal(got["cameras"], np.stack([got["cameras_full"][9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(m)]))


@pytest.mark.parametrize("n,m,p,form", [(3000, 14, 0.5, "slots"), (3000, 14, 0.5, "pairs"), (3001, 12, 1.0, "dense"),
                                         (3001, 14, 0.8, "dense"), (3000, 647, 0.04, None)])
def test_every_schur_form_and_the_646_camera_boundary(n, m, p, form, monkeypatch):
    """The point pass reads records in observation order, so it does not depend on the K3 form (dense with missing
    observations included); 647 cameras: the camera tables leave LDS (k_cam_tables) and D = 5816."""
    if form == "pairs":
        monkeypatch.setenv("MVBA_FORCE_BIG", "1")
    if form is not None:
        monkeypatch.setenv("MVBA_SCHUR", form)
    prob = _problem_from_scene(make_scene(n, m, vis_p=p))
    eng = _engine(prob)
    if form is not None:
        assert eng.schur_info()["kernel"] == form
    got = eng.covariance(full=True)
    # Against the reference on the engine's OWN undamped S (left in the packed [A|b] by the call): the forms of K3 round
    # differently (tests/test_gpu_parity.py holds each to the oracle's S), and S^-1 amplifies that by cond(S) -- the dense
    # form at 3001 x 12 lands 2.7e-8 from the oracle-based reference, the others 6e-11 .. 1.6e-9.  Against that one: 1e-7.
    A = eng.debug_read("A_full").reshape(9 * m, 9 * m)
    A = np.triu(A) + np.triu(A, 1).T
    ref_o = schur_covariance(*prob)
    g = _oracle_linearized(prob)
    sig = np.zeros_like(A)
    sig[np.ix_(g.keep, g.keep)] = np.linalg.inv(A[np.ix_(g.keep, g.keep)])
    ref = {"points": point_blocks(g.E, g.F, prob[2], prob[3], sig), "cameras_full": 2.0 * sig}
    ref["cameras"] = np.stack([ref["cameras_full"][9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(m)])
    for k in ("points", "cameras", "cameras_full"):
        _close(got[k], ref[k], 1e-8, k)
        _close(got[k], ref_o[k], 1e-7, k + " (oracle S)")


def _oracle_linearized(prob):
    from oracle import ba_oracle as O

    n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R = prob
    g = O.OracleEngine(n, m, pt_ptr, cam, xy, f0, axis)
    g.set_params(X, f, u, t, R)
    g.linearize()
    return g


def test_after_optimize_state_frame_and_trajectory(golden):
    d = golden("euclid_default")
    ba = BundleAdjuster(d["x"], d["init_X"], d["init_K"], d["init_R"], d["init_t"], axis="x-up_z-forward")
    ba.optimize(2.0, 1e-8, max_iter=100)
    before = ba._engine.get_params()
    cg = ba.covariance(frame="gauge", full_cameras=True)
    ci = ba.covariance(frame="input", full_cameras=True)
    after = ba._engine.get_params()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)  # the engine's state is restored bitwise
    P, Cc, Cf = covariance_to_input_frame(ba._init_camera0_params, cg["points"], cg["cameras"], cg["cameras_full"])
    assert np.array_equal(ci["points"], P) and np.array_equal(ci["cameras"], Cc) and np.array_equal(ci["cameras_full"], Cf)
    # the gauge-frame blocks are those of the solution mapped back to the gauge frame, computed directly
    ref = schur_covariance(*_gauge_problem_of(ba, d))
    for k in ("points", "cameras", "cameras_full"):
        _close(cg[k], ref[k], 1e-8, k)
    rs = ba.covariance(scale="residual", frame="gauge")
    assert rs["sigma2"] > 0 and np.array_equal(rs["points"], cg["points"] * rs["sigma2"])
    # a covariance between two LM iterations leaves the cost trajectory bitwise as it was
    prob = _problem_from_golden(golden, "euclid_default", "x-up_z-forward")

    def run(with_cov):
        eng = _engine(prob)
        lm, Es = LevenbergMarquardt(eng, 2.0), []
        for i in range(5):
            E_, _ = lm.iterate()
            Es.append(E_)
            if with_cov and i in (1, 2):
                eng.covariance()
            lm.carry_on(E_)
        return Es, eng.get_params()

    (Ea, pa), (Eb, pb) = run(False), run(True)
    assert Ea == Eb
    for a, b in zip(pa, pb):
        assert np.array_equal(a, b)


def _gauge_problem_of(ba, d):
    from lib.bundle_adjustment import from_gauge_frame_inverse

    X, f, u, t, R = ba._engine.get_params()
    Xg, Rg, tg = from_gauge_frame_inverse(ba._init_camera0_params, X, R, t)
    pt_ptr, cam, xy = dense_to_observations(d["x"], None)
    xy = np.ascontiguousarray(xy.transpose(1, 0, 2).reshape(-1, 2)) if xy.ndim == 3 else xy
    return (d["x"].shape[0], d["x"].shape[1], pt_ptr, cam, xy, 1.0, "x-up_z-forward", Xg, f, u, tg, Rg)


def test_two_calls_are_bitwise_identical():
    eng = _engine(_problem_from_scene(make_scene(2000, 12, vis_p=0.4)))
    a, b = eng.covariance(full=True), eng.covariance(full=True)
    for k in ("points", "cameras", "cameras_full"):
        assert np.array_equal(a[k], b[k]), k


def test_point_seen_once_raises_and_the_engine_still_optimises():
    sc = make_scene(300, 8, vis_p=0.6)
    n, m = sc.n_points, sc.n_images
    deg = np.diff(sc.pt_ptr)
    keep = np.ones(len(sc.cam_idx), bool)
    keep[sc.pt_ptr[5] + 1:sc.pt_ptr[6]] = False  # point 5 keeps its first observation only
    pt_ptr = np.concatenate([[0], np.cumsum(np.where(np.arange(n) == 5, 1, deg))])
    X, R, t = to_gauge_frame(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    prob = (n, m, pt_ptr, sc.cam_idx[keep], sc.xy[keep], 1.0, sc.axis, X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    eng = _engine(prob)
    with pytest.raises(np.linalg.LinAlgError):
        eng.covariance()
    E0 = eng.cost()
    E = lm_loop(eng, 2.0, -1.0, 5, verbose=False)
    assert np.isfinite(E) and E < E0


def test_two_thread_ranks_host_transport():
    from lib import _distributed as D

    sc = make_scene(3000, 20, vis_p=0.3)
    prob = _problem_from_scene(sc)
    n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R = prob
    one = _engine(prob).covariance(full=True)
    parts = D.partition_points(pt_ptr, 2)

    def body(rank, g):
        from lib._mvba import HipEngine

        lo, hi = parts[rank]
        p2, c2, x2 = D.slice_observations(pt_ptr, cam, xy, lo, hi)
        eng = HipEngine(hi - lo, m, p2, c2, x2, f0, axis)
        g.attach(eng, rank)
        eng.set_params(X[lo:hi], f, u, t, R)
        return eng.covariance(full=True)

    res = D.InProcessGroup(2).run(body)
    for k in ("cameras", "cameras_full"):
        assert np.array_equal(res[0][k], res[1][k]), k
        _close(res[0][k], one[k], 1e-10, k)
    _close(np.concatenate([r["points"] for r in res]), one["points"], 1e-10, "points")


def test_config3_full_size():
    """1 M points x 100 cameras x 10 %: finite, symmetric, positive semi-definite blocks; 1000 sampled points against the
    point formula evaluated in NumPy from the engine's own camera covariance, E_a and records."""
    m = 100
    sc = make_scene(1_000_000, m, vis_p=0.1)
    prob = _problem_from_scene(sc)
    eng = _engine(prob)
    got = eng.covariance(full=True)
    P, Cc, Cf = got["points"], got["cameras"], got["cameras_full"]
    for A in (P, Cc):
        assert np.isfinite(A).all()
        assert np.array_equal(A, A.transpose(0, 2, 1))
        w = np.linalg.eigvalsh(A)
        assert (w >= -1e-12 * np.abs(w).max(axis=1, keepdims=True)).all()
    assert np.array_equal(Cf, Cf.T)
    # the NumPy evaluation: Sigma = C_full / 2, E_a from the engine, F_o = 2 Jx^T Jc from the engine's records
    rng = np.random.default_rng(11)
    pts = np.sort(rng.choice(sc.n_points, 1000, replace=False))
    E6 = eng.debug_read("E").reshape(-1, 6)
    JX = eng.debug_read("JX").reshape(-1, 2, 3)
    JC = eng.debug_read("JC").reshape(-1, 2, 9)
    iu = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    E = E6[:, iu]
    sel = np.concatenate([np.arange(sc.pt_ptr[a], sc.pt_ptr[a + 1]) for a in pts])  # the sampled points as a CSR of their own
    sub_ptr = np.concatenate([[0], np.cumsum(np.diff(sc.pt_ptr)[pts])])
    F = 2.0 * np.einsum("ori,orj->oij", JX[sel], JC[sel])
    ref = point_blocks(E[pts], F, sub_ptr, sc.cam_idx[sel], Cf / 2.0)
    _close(P[pts], ref, 1e-9, "sampled points")
    t = got["timings_ms"]
    print("config 3 covariance ms:", t)
