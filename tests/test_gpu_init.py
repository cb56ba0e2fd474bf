"""Initial estimates on the device: mvba_triangulate, mvba_triangulate_state and mvba_resect against the NumPy
restatement of tests/_init_ref.py.  Parity margins: 100 x the host-versus-host difference (eigh against SVD) of the very
scene, recorded in tests/_init_cases.py and re-measured by tests/test_init_cpu.py."""
import ctypes as C_
import os
import subprocess
import sys

import numpy as np
import pytest

import _init_cases as C
import _init_ref as ref
from _engines import HostOracleEngine
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster, dense_to_observations, intrinsics_from, to_gauge_frame
from lib.initialization import resect_cameras, triangulate_points
from lib.synthetic import make_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, want, margin, what):
    """max |got - want| <= margin, NaN where the reference is NaN; prints the figure before it asserts."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    fin = ~np.isnan(want)
    d = np.abs(got[fin] - want[fin])
    print(f"{what}: max abs difference {d.max() if d.size else 0.0:.3e} (margin {margin:.1e})")
    assert (d <= margin).all(), (what, d.max(), margin)


@pytest.mark.parametrize("n_refine", [0, 2])
@pytest.mark.parametrize("name", sorted(C.TRI_HOST_DIFF))
def test_triangulate_parity(name, n_refine):
    K, R, t, pt_ptr, cam_idx, xy = C.tri_args(name)
    X, q, st, tm = _mvba.triangulate(K, R, t, pt_ptr, cam_idx, xy, n_refine=n_refine)
    Xr, qr, sr = C.tri_reference(name, n_refine)
    np.testing.assert_array_equal(st, sr)
    assert (st == 0).all() and X.shape == Xr.shape  # no point may be left out
    margin = C.MARGIN * C.TRI_HOST_DIFF[name]  # 100 x the host-versus-host difference of this scene's linear step
    _close(X, Xr, margin, f"{name} n_refine={n_refine} X")
    _close(q, qr, margin, f"{name} n_refine={n_refine} quality")
    assert set(tm) == {"upload", "kernel", "download"} and tm["kernel"] > 0


def test_project_of_triangulate_returns_the_observations():
    sc = make_scene(300, 8, vis_p=0.5, noise=0.0, project="numpy")
    xy = C.exact_xy(sc)
    X, info = triangulate_points(sc.pt_ptr, sc.cam_idx, xy, sc.K_gt, sc.R_gt, sc.t_gt)
    assert (info["status"] == 0).all()
    back = _mvba.project(X, sc.K_gt, sc.R_gt, sc.t_gt, sc.pt_ptr, sc.cam_idx)
    np.testing.assert_allclose(back, xy, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(X, sc.X_gt, rtol=0, atol=1e-12)


def test_triangulate_status_cases():
    K, R, t, pt_ptr, cam, xy, expect, X_gt = C.status_case()
    for n_refine in (0, 2):
        X, q, st, _ = _mvba.triangulate(K, R, t, pt_ptr, cam, xy, n_refine=n_refine)
        np.testing.assert_array_equal(st, expect)
        bad = expect != 0
        assert np.isnan(X[bad]).all() and np.isnan(q[bad]).all()
        np.testing.assert_allclose(X[~bad], X_gt[~bad], rtol=0, atol=1e-12)  # the neighbours are unaffected
        assert np.isfinite(q[~bad]).all()


def test_triangulate_and_resect_are_bitwise_deterministic():
    a = _mvba.triangulate(*C.tri_args("300x8"))
    b = _mvba.triangulate(*C.tri_args("300x8"))
    for u, v in zip(a[:3], b[:3]):
        assert u.tobytes() == v.tobytes()
    X, pt_ptr, cam, xy, m, _ = C.resect_case("5000x3")
    a, b = _mvba.resect(X, pt_ptr, cam, xy, m), _mvba.resect(X, pt_ptr, cam, xy, m)
    for u, v in zip(a[:3], b[:3]):
        assert u.tobytes() == v.tobytes()


def _gauge_cameras(sc):
    _, R, t = to_gauge_frame(np.zeros((0, 3)), sc.init_R, sc.init_t, sc.axis)
    return sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R


@pytest.mark.parametrize("loss", ["squared", "huber"])
def test_engine_triangulate_equals_the_stateless_call(loss):
    sc = C.tri_scene("300x8")
    f, u, t, R = _gauge_cameras(sc)
    kw = {} if loss == "squared" else {"loss": loss, "loss_scale": 2e-3}
    eng = _mvba.HipEngine(sc.n_points, 8, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis, **kw)
    X0 = np.full((sc.n_points, 3), 7.0)
    eng.set_params(X0, f, u, t, R)
    q, st, tm = eng.triangulate(2)
    X = eng.get_params()[0]
    X1, q1, st1, _ = _mvba.triangulate(intrinsics_from(f, u, 1.0), R, t, sc.pt_ptr, sc.cam_idx, sc.xy, n_refine=2)
    margin = C.MARGIN * C.TRI_HOST_DIFF["300x8"]
    np.testing.assert_array_equal(st, st1)
    assert (st == 0).all() and tm["upload"] == 0.0
    _close(X, X1, margin, f"engine ({loss}) X against the stateless call")
    _close(q, q1, margin, f"engine ({loss}) quality")
    Xr, _, _ = ref.triangulate(intrinsics_from(f, u, 1.0), R, t, sc.pt_ptr, sc.cam_idx, sc.xy, 2)
    _close(X, Xr, margin, f"engine ({loss}) X against the reference")
    # the linearisation and the trial are void afterwards, as after set_params
    eng.linearize()
    eng.try_step(1e-4)
    eng.triangulate(2)
    with pytest.raises(RuntimeError, match="libmvba error 5"):
        eng.try_step(1e-4)
    with pytest.raises(RuntimeError, match="libmvba error 5"):
        eng.commit()
    eng.linearize()
    assert np.isfinite(eng.try_step(1e-4))
    eng.close()


def test_engine_triangulate_in_pixel_units():
    """f0 = 600, raw pixel observations: the engine-resident form must agree with the engine's own residual
    (p / r - x / f0): the committed points are the reference's for the matrix that projects to raw pixels, the RMS residual is
    in pixels, and the engine's cost at them is the oracle's."""
    from oracle import ba_oracle as O

    sc, xy_px, K, K_raw = C.pixel_scene()
    _, R, t = to_gauge_frame(np.zeros((0, 3)), sc.init_R, sc.init_t, sc.axis)
    f, u = K[:, 0, 0], K[:, :2, 2]
    eng = _mvba.HipEngine(sc.n_points, 8, sc.pt_ptr, sc.cam_idx, xy_px, C.PIXEL_F0, sc.axis)
    eng.set_params(np.zeros((sc.n_points, 3)), f, u, t, R)
    q, st, _ = eng.triangulate(2)
    X = eng.get_params()[0]
    Xr, qr, sr = ref.triangulate(K_raw, R, t, sc.pt_ptr, sc.cam_idx, xy_px, 2)
    assert (st == 0).all() and (sr == 0).all()
    margin = C.MARGIN * C.TRI_HOST_DIFF["pixels"]
    _close(X, Xr, margin, "pixels engine X")
    _close(q, qr, margin, "pixels engine quality")
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    e = O.residuals(Xr, f, u, t, R, C.PIXEL_F0, pt, sc.cam_idx, xy_px)
    E, E_ref = eng.cost(), float((e * e).sum())
    print("pixels cost", E, E_ref)
    assert abs(E - E_ref) <= 1e-9 * E_ref
    # small: the cameras are the truth perturbed by 0.01, the residuals (units x / f0) of that order -- not the thousands of a
    # projection that is off by a factor f0
    assert E / sc.n_obs < 1e-3
    np.testing.assert_allclose(np.sqrt((q[:, 0] ** 2 * np.diff(sc.pt_ptr)).sum()), C.PIXEL_F0 * np.sqrt(E), rtol=1e-9)  # RMS in pixels
    eng.close()


def test_from_observations_init_X_none_in_pixel_units():
    sc, xy_px, K, K_raw = C.pixel_scene()
    ba = BundleAdjuster.from_observations(sc.n_points, 8, sc.pt_ptr, sc.cam_idx, xy_px, None, K, sc.init_R, sc.init_t,
                                          f0=C.PIXEL_F0, axis=sc.axis)
    _, Rg, tg = to_gauge_frame(np.zeros((0, 3)), sc.init_R, sc.init_t, sc.axis)
    Xr, _, sr = ref.triangulate(K_raw, Rg, tg, sc.pt_ptr, sc.cam_idx, xy_px, 2)
    assert (sr == 0).all()
    _close(ba._engine.get_params()[0], Xr, C.MARGIN * C.TRI_HOST_DIFF["pixels"], "pixels from_observations X")
    E0 = ba._engine.cost()
    assert E0 / sc.n_obs < 1e-3
    X, Ko, Ro, to = ba.optimize(2.0, -1.0, 5)
    E1 = ba._engine.cost()
    assert E1 < 0.1 * E0  # BA goes on from there: from residuals of the camera perturbation (1e-2) to those of the noise (1e-3)
    # resect_cameras on raw pixels gives the adjuster's init_K back (noise-free: the cameras that made the observations)
    scn, xyn, Kn, _ = C.pixel_scene(noise_free=True)
    K2, R2, t2, info = resect_cameras(scn.X_gt, scn.pt_ptr, scn.cam_idx, xyn, 8, f0=C.PIXEL_F0)
    assert (info["status"] == 0).all()
    np.testing.assert_allclose(K2, Kn, rtol=0, atol=1e-7)
    np.testing.assert_allclose(R2, scn.R_gt, rtol=0, atol=1e-10)
    np.testing.assert_allclose(t2, scn.t_gt, rtol=0, atol=1e-9)


def test_engine_triangulate_keeps_the_points_it_cannot_do():
    K, R, t, pt_ptr, cam, xy, expect, X_gt = C.status_case()
    eng = _mvba.HipEngine(40, 4, pt_ptr, cam, xy, 1.0, "x-up_z-forward")
    eng.set_params(np.full((40, 3), 7.0), K[:, 0, 0], K[:, :2, 2], t, R)
    q, st, _ = eng.triangulate(2)
    X = eng.get_params()[0]
    np.testing.assert_array_equal(st, expect)
    assert (X[expect != 0] == 7.0).all() and np.isnan(q[expect != 0]).all()
    np.testing.assert_allclose(X[expect == 0], X_gt[expect == 0], rtol=0, atol=1e-12)
    eng.close()


def test_engine_triangulate_world_size_2_on_one_gpu():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", "29561", os.path.join(ROOT, "tests", "_dist_init_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_INIT_OK" in out.stdout


@pytest.mark.parametrize("name", ["300x8", "5000x3", "six", "dense", "coplanar", "900x300", "edges"])
def test_resect_parity(name):
    X, pt_ptr, cam, xy, m, expect = C.resect_case(name)
    print(f"{name}: {int((expect == 1).sum())} of {m} cameras have fewer than 6 observations")
    if name == "dense":  # the dense grid from Python: no list, xy (N, m, 2)
        P, q, st, tm = _mvba.resect(X, None, None, xy.reshape(len(X), m, 2), m)
    else:
        P, q, st, tm = _mvba.resect(X, pt_ptr, cam, xy, m)
    Pr, qr, sr = C.resect_reference(name)
    np.testing.assert_array_equal(st, sr)
    np.testing.assert_array_equal(st, expect)
    assert np.isnan(P[st != 0]).all() and np.isnan(q[st != 0, 0]).all() and np.isnan(q[st == 1, 1]).all()
    good = st == 0
    if good.any():
        margin = C.MARGIN * C.RESECT_HOST_DIFF[name]  # 100 x the host-versus-host difference of this scene
        _close(P.reshape(m, 12)[good], Pr[good], margin, f"{name} P")
        _close(q[good], qr[good], margin, f"{name} quality")
        np.testing.assert_allclose(np.linalg.norm(P[good][:, 2, :3], axis=1), 1.0, rtol=0, atol=1e-14)
        assert (np.linalg.det(P[good][:, :, :3]) > 0).all()
    assert tm["kernel"] > 0


def test_resect_honours_point_ok_and_resect_cameras_decomposes():
    X, pt_ptr, cam, xy, m, _ = C.resect_case("300x8")
    ok = np.random.default_rng(5).random(len(X)) < 0.6
    P, q, st, _ = _mvba.resect(X, pt_ptr, cam, xy, m, point_ok=ok)
    Pr, qr, sr = ref.resect(X, pt_ptr, cam, xy, m, point_ok=ok)
    Ps, _, _ = ref.resect(X, pt_ptr, cam, xy, m, point_ok=ok, linear="svd")
    np.testing.assert_array_equal(st, sr)
    _close(P.reshape(m, 12), Pr, C.MARGIN * np.abs(Ps - Pr).max(), "masked P")  # (this list's own host-versus-host difference)
    Xn = np.where(ok[:, None], X, np.nan)
    P2 = _mvba.resect(Xn, pt_ptr, cam, xy, m)[0]  # the default mask: the points whose X is finite
    assert P2.tobytes() == P.tobytes()
    assert not np.array_equal(P, _mvba.resect(X, pt_ptr, cam, xy, m)[0])
    # noise-free: resect_cameras returns the cameras that made the observations
    sc = make_scene(300, 8, vis_p=0.5, noise=0.0, project="numpy")
    K, R, t, info = resect_cameras(sc.X_gt, sc.pt_ptr, sc.cam_idx, C.exact_xy(sc), 8)
    assert (info["status"] == 0).all()
    np.testing.assert_allclose(K, sc.K_gt, rtol=0, atol=1e-10)
    np.testing.assert_allclose(R, sc.R_gt, rtol=0, atol=1e-10)
    np.testing.assert_allclose(t, sc.t_gt, rtol=0, atol=1e-10)


class _OracleBackedAdjuster(BundleAdjuster):
    """The product's host LM loop over the CPU oracle engine (tests/test_host_cpu.py)."""

    def _make_engine(self, n_points, n_images, pt_ptr, cam_idx, xy, f0, axis, **kw):
        return HostOracleEngine(n_points, n_images, pt_ptr, cam_idx, np.asarray(xy).reshape(-1, 2), f0, axis)


def test_bundle_adjustment_from_triangulated_points(golden):
    d = golden("visibility_300x12")
    axis, args = "x-up_z-forward", (2.0, -1.0, 10)
    pt_ptr, cam_idx, xy = dense_to_observations(d["x"], d["vis"])
    K, R, t = d["init_K"], d["init_R"], d["init_t"]
    ba = BundleAdjuster.from_observations(300, 12, pt_ptr, cam_idx, xy, None, K, R, t, axis=axis)
    X, Ko, Ro, to = ba.optimize(*args, is_debug=True)
    E = np.array([e["reprojection_error"] for e in ba.get_log()])
    # the oracle starts from the reference-triangulated points: the same computation, in the gauge frame the engine holds
    _, Rg, tg = to_gauge_frame(np.zeros((0, 3)), R, t, axis)
    Xg, _, st = ref.triangulate(intrinsics_from(K[:, 0, 0], K[:, :2, 2], 1.0), Rg, tg, pt_ptr, cam_idx, xy, 2)
    assert (st == 0).all()
    s = np.sign((t[1] - t[0])[1]) * (R[0][:, 1] @ (t[1] - t[0]))  # the divisor of to_gauge_frame (signed: SURVEY B.2)
    X_in = t[0] + (s * Xg) @ R[0].T  # its inverse: the adjuster's own to_gauge_frame hands the oracle Xg again
    oba = _OracleBackedAdjuster.from_observations(300, 12, pt_ptr, cam_idx, xy, X_in, K, R, t, axis=axis)
    X2, K2, R2, t2 = oba.optimize(*args, is_debug=True)
    E2 = np.array([e["reprojection_error"] for e in oba.get_log()])
    assert len(E) == len(E2) and ba._engine.n_solves == oba._engine.n_solves  # the same outer and inner iteration counts
    print("E", E, "max |dX|", np.abs(X - X2).max())
    np.testing.assert_allclose(E, E2, rtol=1e-9, atol=1e-12)  # (the tolerances of tests/test_gpu_parity.py for a trajectory)
    for got, want in ((X, X2), (Ko, K2), (Ro, R2), (to, t2)):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    assert E[-1] < E[0]
    # the dense constructor takes init_X=None the same way
    ba2 = BundleAdjuster(d["x"], None, K, R, t, visibility_index=d["vis"], axis=axis)
    assert np.array_equal(ba2._engine.get_params()[0], BundleAdjuster.from_observations(
        300, 12, pt_ptr, cam_idx, xy, None, K, R, t, axis=axis)._engine.get_params()[0])


def test_init_X_none_with_an_untriangulable_point_is_a_value_error(golden):
    d = golden("visibility_300x12")
    pt_ptr, cam_idx, xy = dense_to_observations(d["x"], d["vis"])
    keep = np.ones(len(cam_idx), bool)
    keep[pt_ptr[17] + 1:pt_ptr[18]] = False  # point 17 keeps one observation
    deg = np.diff(pt_ptr)
    deg[17] = 1
    p2 = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    with pytest.raises(ValueError, match=r"1 of 300 points.*first: point 17, status 1"):
        BundleAdjuster.from_observations(300, 12, p2, cam_idx[keep], xy[keep], None, d["init_K"], d["init_R"], d["init_t"],
                                         axis="x-up_z-forward")


def test_c_abi_argument_errors():
    lib = _mvba.load_library()
    K, R, t, pt_ptr, cam, xy = C.tri_args("300x8")
    n, m, n_obs = len(pt_ptr) - 1, 8, len(cam)
    dp, ip, lp = _mvba._ptr, (lambda a: a.ctypes.data_as(C_.POINTER(C_.c_int32))), (lambda a: a.ctypes.data_as(C_.POINTER(C_.c_int64)))
    X = np.empty((n, 3))

    def tri(K=K, pt_ptr=pt_ptr, cam=cam, m=m, n_obs=n_obs, X=X, n_refine=2, Kp=None):
        rc = lib.mvba_triangulate(Kp if K is None else dp(K), dp(R), dp(t), m, n, lp(pt_ptr) if pt_ptr is not None else None, ip(cam), dp(xy),
                                  n_obs, n_refine, dp(X) if X is not None else None, None, None, None, -1)
        return rc, lib.mvba_last_error().decode()

    assert tri()[0] == _mvba.MVBA_OK
    rc, msg = tri(K=None)
    assert rc == _mvba.MVBA_ERR_BADARG and "null argument: K (argument 1)" in msg
    rc, msg = tri(X=None)
    assert rc == _mvba.MVBA_ERR_BADARG and "X (argument 11)" in msg
    bad = cam.copy()
    bad[41] = 8
    rc, msg = tri(cam=bad)
    assert rc == _mvba.MVBA_ERR_BADARG and "cam_idx[41] = 8" in msg and "n_images = 8" in msg
    bad[41] = -1
    assert tri(cam=bad)[0] == _mvba.MVBA_ERR_BADARG
    rc, msg = tri(n_obs=n_obs - 1)
    assert rc == _mvba.MVBA_ERR_BADARG and str(n_obs - 1) in msg
    p2 = pt_ptr.copy()
    p2[5] = p2[6] + 1  # not ascending
    rc, msg = tri(pt_ptr=p2)
    assert rc == _mvba.MVBA_ERR_BADARG and "pt_ptr[6]" in msg
    rc, msg = tri(m=1705)
    assert rc == _mvba.MVBA_ERR_BADARG and ("1705" in msg)
    rc, msg = tri(n_refine=-1)
    assert rc == _mvba.MVBA_ERR_BADARG and "n_refine = -1" in msg
    rc, msg = tri(pt_ptr=None)  # the dense grid needs n_obs = n_points * n_images
    assert rc == _mvba.MVBA_ERR_BADARG and str(n * m) in msg
    # too many cameras for the LDS table: a list that is otherwise valid
    m_big = 1705
    Kb, Rb, tb = np.tile(np.eye(3), (m_big, 1, 1)), np.tile(np.eye(3), (m_big, 1, 1)), np.zeros((m_big, 3))
    rc = lib.mvba_triangulate(dp(Kb), dp(Rb), dp(tb), m_big, n, lp(pt_ptr), ip(cam), dp(xy), n_obs, 0, dp(X), None, None, None, -1)
    assert rc == _mvba.MVBA_ERR_BADARG and "n_images = 1705 (max 1704)" in lib.mvba_last_error().decode()
    # mvba_resect
    Xg, P = C.tri_scene("300x8").X_gt, np.empty((m, 12))

    def res(X=Xg, cam=cam, n_obs=n_obs, P=P):
        rc = lib.mvba_resect(dp(X) if X is not None else None, n, lp(pt_ptr), ip(cam), dp(xy), n_obs, m, None, dp(P) if P is not None else None,
                             None, None, None, -1)
        return rc, lib.mvba_last_error().decode()

    assert res()[0] == _mvba.MVBA_OK
    rc, msg = res(X=None)
    assert rc == _mvba.MVBA_ERR_BADARG and "X (argument 1)" in msg
    rc, msg = res(P=None)
    assert rc == _mvba.MVBA_ERR_BADARG and "P (argument 9)" in msg
    bad[41] = 9
    rc, msg = res(cam=bad)
    assert rc == _mvba.MVBA_ERR_BADARG and "cam_idx[41] = 9" in msg
    rc, msg = res(n_obs=n_obs + 3)
    assert rc == _mvba.MVBA_ERR_BADARG and str(n_obs + 3) in msg
    # mvba_triangulate_state
    assert lib.mvba_triangulate_state(None, 2, None, None, None) == _mvba.MVBA_ERR_BADARG
    sc = C.tri_scene("300x8")
    eng = _mvba.HipEngine(sc.n_points, 8, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis)
    with pytest.raises(RuntimeError, match="libmvba error 5"):  # no cameras committed yet
        eng.triangulate()
    with pytest.raises(ValueError, match="n_refine = -2"):
        eng.triangulate(-2)
    eng.close()
