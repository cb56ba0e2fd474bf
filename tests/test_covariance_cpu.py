"""Marginal covariances, host side (no GPU): the Schur-based reference against the dense inverse, the map from the gauge
frame to the input frame, and the residual variance."""
import numpy as np
import pytest

from _covariance_ref import dense_covariance, dense_covariance_extended, schur_covariance, schur_covariance_extended
from lib.bundle_adjustment import (camera_frame_map, covariance_to_input_frame, dense_to_observations, from_gauge_frame,
                                   from_gauge_frame_inverse, residual_variance, to_gauge_frame)
from lib.synthetic import make_scene
from oracle import ba_oracle as O


def _close(a, b, tol):
    scale = np.abs(b).max()
    assert np.abs(a - b).max() <= tol * scale, (np.abs(a - b).max(), scale)


def _golden_problem(golden):
    d = golden("linearize_60x7_xright")
    x, vis = d["x"], d["vis"]
    pt_ptr, cam, xy = dense_to_observations(x, vis)
    axis = str(d["axis"])
    return (x.shape[0], x.shape[1], pt_ptr, cam, xy, 1.0, axis, d["norm_X"], d["f"], d["u"], d["norm_t"], d["norm_R"])


def _scene_problem(n, m, vis):
    sc = make_scene(n, m, vis_p=vis, project="numpy")
    X, R, t = to_gauge_frame(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    return (sc.n_points, m, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis, X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)


# (the golden 60 x 7 scene at its initial state has cond(J) = 7e5: the Schur form works on the normal equations, whose
# condition number is the square of that, and agrees with the QR-based inverse to 4.5e-10 there; cond(J) = 1.5e4 for the
# synthetic scene)
@pytest.mark.parametrize("which,tol", [("golden_60x7", 2e-9), ("scene_200x6", 1e-10)])
def test_schur_reference_equals_dense_inverse(golden, which, tol):
    prob = _golden_problem(golden) if which == "golden_60x7" else _scene_problem(200, 6, 0.7)
    d, s = dense_covariance(*prob), schur_covariance(*prob)
    for k in ("points", "cameras", "cameras_full"):
        _close(s[k], d[k], tol)
    removed = O.gauge_removed(prob[6])
    assert not d["cameras_full"][removed].any() and not d["cameras_full"][:, removed].any()


def test_schur_construction_equals_dense_inverse_to_1e10_in_extended_precision(golden):
    """The 60 x 7 golden scene at 1e-10: the double-precision gap above is the rounding of the normal equations (J^T J formed
    in double at cond 5e11), not the Schur formulas -- the same two constructions in long double agree to 4.5e-12, and the
    double QR-based inverse is within 4.7e-12 of them."""
    prob = _golden_problem(golden)
    a, b, d = dense_covariance_extended(*prob), schur_covariance_extended(*prob), dense_covariance(*prob)
    for k in ("points", "cameras_full"):
        _close(b[k], a[k], 1e-10)
        _close(d[k].astype(np.longdouble), a[k], 1e-10)


def _cam0(seed=3):
    rng = np.random.default_rng(seed)
    R0, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return {"R": R0, "t": rng.normal(size=3), "c0c1_len": 2.7}


def test_input_frame_map_matches_explicit_T():
    cam0 = _cam0()
    rng = np.random.default_rng(5)
    m, n = 4, 6
    B = rng.normal(size=(9 * m, 9 * m))
    full = B @ B.T
    removed = O.gauge_removed("x-right_z-forward")
    full[removed] = 0.0
    full[:, removed] = 0.0
    cams = np.stack([full[9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(m)])
    P = rng.normal(size=(n, 3, 3))
    P = P @ P.transpose(0, 2, 1)
    R0, L = cam0["R"], cam0["c0c1_len"]
    T = np.zeros((9, 9))
    T[:3, :3] = np.eye(3)
    T[3:6, 3:6] = L * R0
    T[6:, 6:] = R0
    np.testing.assert_allclose(camera_frame_map(cam0), T, rtol=0, atol=1e-15)
    Tb = np.kron(np.eye(m), T)
    Pi, Ci, Fi = covariance_to_input_frame(cam0, P, cams, full)
    np.testing.assert_allclose(Fi, Tb @ full @ Tb.T, rtol=1e-12, atol=1e-12 * np.abs(full).max())
    for k in range(m):
        np.testing.assert_allclose(Ci[k], T @ cams[k] @ T.T, rtol=1e-12, atol=1e-12 * np.abs(cams).max())
    for a in range(n):
        np.testing.assert_allclose(Pi[a], L * L * R0 @ P[a] @ R0.T, rtol=1e-12, atol=1e-12 * np.abs(P).max())
    assert not Ci[0][3:, :].any() and not Ci[0][:, 3:].any()  # camera 0's t and omega: fixed by the gauge in either frame
    assert not Fi[3:9].any() and not Fi[:, 3:9].any()


def test_input_frame_map_is_the_linearisation_of_from_gauge_frame():
    """T is the Jacobian of the way back: a small gauge-frame step in t and omega moves the input-frame pose by T times it."""
    cam0 = _cam0(7)
    rng = np.random.default_rng(8)
    X = rng.normal(size=(5, 3))
    R = np.stack([O.rodrigues(w) for w in rng.normal(size=(2, 3))])
    t = rng.normal(size=(2, 3))
    dt, dw = 1e-7 * rng.normal(size=3), 1e-7 * rng.normal(size=3)
    _, Ra, ta = from_gauge_frame(cam0, X, R, t)
    t2, R2 = t.copy(), R.copy()
    t2[1] += dt
    R2[1] = O.rodrigues(dw) @ R[1]
    _, Rb, tb = from_gauge_frame(cam0, X, R2, t2)
    T = camera_frame_map(cam0)
    np.testing.assert_allclose(tb[1] - ta[1], T[3:6, 3:6] @ dt, rtol=0, atol=1e-15)
    W = Rb[1] @ Ra[1].T  # = Rod(omega_in)
    w_in = np.array([W[2, 1] - W[1, 2], W[0, 2] - W[2, 0], W[1, 0] - W[0, 1]]) / 2
    np.testing.assert_allclose(w_in, T[6:, 6:] @ dw, rtol=1e-6, atol=1e-20)
    Xg, Rg, tg = from_gauge_frame_inverse(cam0, *from_gauge_frame(cam0, X, R, t))
    np.testing.assert_allclose(Xg, X, atol=1e-13)
    np.testing.assert_allclose(tg, t, atol=1e-13)
    np.testing.assert_allclose(Rg, R, atol=1e-13)


def test_residual_variance():
    assert residual_variance(3.0, 100, 20, 5) == 3.0 / (200 - (60 + 45 - 7))
    with pytest.raises(ValueError):
        residual_variance(1.0, 10, 5, 2)  # 20 - (15 + 18 - 7) < 0
    with pytest.raises(ValueError):
        residual_variance(1.0, 13, 5, 2)  # exactly zero redundancy
