"""Two-view start, the part that needs no GPU: the host-versus-host differences that set the GPU parity margins
are what tests/_twoview_cases.py records, the NumPy reference of tests/_twoview_ref.py recovers the ground truth of a
noise-free scene and grows the issue's scene into a full reconstruction, and libmvba.so exports the new entry points."""
import ctypes
import os

import numpy as np
import pytest

import _twoview_cases as C
import _twoview_ref as T
from lib import _mvba
from lib.initialization import engine_intrinsics, pose_candidates, pose_for_intrinsics, restrict_observations


@pytest.mark.parametrize("name", sorted(C.TWOVIEW_HOST_DIFF))
def test_fundamental_host_versus_host_difference(name):
    """eigh(M) against the SVD of the stacked rows: the figure the GPU parity margin is 100 x of."""
    a, b = C.reference(name), C.reference(name, "svd")
    np.testing.assert_array_equal(a[3], b[3])
    np.testing.assert_array_equal(a[2], b[2])
    ok = a[3] == 0
    d = np.abs(a[0][ok] - b[0][ok]).max()
    rel = (np.abs(a[1][ok, 0] - b[1][ok, 0]) / a[1][ok, 0])[a[2][ok] > 8].max()
    print(f"{name}: eigh vs SVD max |dF| = {d:.3e} (recorded {C.TWOVIEW_HOST_DIFF[name]:.1e}), Sampson RMS relative {rel:.3e}")
    assert 0.5 * C.TWOVIEW_HOST_DIFF[name] <= d <= C.TWOVIEW_HOST_DIFF[name]
    assert rel <= C.MARGIN * C.TWOVIEW_HOST_DIFF[name]  # (the Sampson RMS under the same relative margin)
    F = a[0][ok]
    np.testing.assert_allclose(np.linalg.norm(F, axis=(1, 2)), 1.0, rtol=0, atol=1e-14)
    assert (np.abs(np.linalg.det(F)) < 1e-15).all()  # rank 2: |F| = 1, so det = s1 s2 s3 with s3 = 0 up to rounding
    assert (F.reshape(len(F), 9)[np.arange(len(F)), np.abs(F.reshape(len(F), 9)).argmax(axis=1)] > 0).all()


def test_issue_scenes_have_the_stated_counts():
    ns, st = C.reference("300x8")[2:]
    assert ns[:28].max() == 90 and ns[:28].min() == 67 and (st == 0).all()
    ns, st = C.reference("65x12")[2:]
    assert (ns == 7).any() and (ns == 8).any()
    np.testing.assert_array_equal(st, np.where(ns < 8, 1, 0))
    q = C.reference("65x12")[1]
    assert np.isnan(C.reference("65x12")[0][st == 1]).all() and np.isnan(q[st == 1]).all()
    assert 0.03 < q[st == 0, 1].max() < 0.05  # lambda_1 / lambda_2 up to 0.04


def test_reversed_pair_is_the_transpose():
    F = C.reference("300x8")[0]
    pairs = [tuple(p) for p in C.case("300x8")[4]]
    for rev in ((5, 2), (7, 0)):
        a, b = F[pairs.index(rev)], F[pairs.index(rev[::-1])]
        np.testing.assert_allclose(a, b.T, rtol=0, atol=C.MARGIN * C.TWOVIEW_HOST_DIFF["300x8"])


def test_reference_against_the_true_essential_matrix_and_pose():
    """Noise-free, K_gt = I: F = E up to scale and sign; exactly one of the four pose candidates puts every shared point in
    front of both cameras, and it is the ground truth.  Re-measures the three figures the GPU pose margin is made of."""
    sc = C.scene("noise_free")
    pairs = C.all_pairs(8)
    F, q, ns, st = C.reference("noise_free")
    assert (st == 0).all()
    err = max(np.abs(F[i] - C.true_essential(sc, k, l)).max() for i, (k, l) in enumerate(pairs))
    print(f"max |F - E_gt| over 28 pairs = {err:.3e}")
    assert err < 1e-11  # measured 7.4e-13
    assert q[:, 0].max() < 1e-14 and np.abs(q[:, 1]).max() < 1e-12
    f_host = np.abs(F[0] - C.reference("noise_free", "svd")[0][0]).max()
    f_err = np.abs(F[0] - C.true_essential(sc, 0, 1)).max()
    for i, (k, l) in enumerate(pairs):
        R, t, X, info = T.relative_pose(sc.pt_ptr, sc.cam_idx, sc.xy, sc.K_gt, (k, l), F=F[i])
        assert info["status"] == 0 and sorted(info["n_front"]) == [0, 0, 0, ns[i]], info["n_front"]
        Rg, tg = C.true_relative_pose(sc, k, l)
        e = max(np.abs(R[1] - Rg).max(), np.abs(t[1] - tg).max())
        assert e < 1e-11
        ids = np.isfinite(X).all(axis=1)
        assert ids.sum() == ns[i]
        if (k, l) == (0, 1):
            print(f"pair (0, 1): host-vs-host |dF| {f_host:.3e}, |F - E_gt| {f_err:.3e}, pose error {e:.3e}")
            assert 0.5 * C.POSE_F_HOST_DIFF <= f_host <= C.POSE_F_HOST_DIFF
            assert 0.5 * C.POSE_REF_F_ERR <= f_err <= C.POSE_REF_F_ERR and 0.5 * C.POSE_REF_POSE_ERR <= e <= C.POSE_REF_POSE_ERR
            s = np.linalg.norm(sc.t_gt[1] - sc.t_gt[0])
            np.testing.assert_allclose(X[ids], ((sc.X_gt - sc.t_gt[0]) @ sc.R_gt[0])[ids] / s, rtol=0, atol=1e-11)


def test_degenerate_pairs_have_status_2():
    for name in ("planar", "same_centre"):
        pt_ptr, cam, xy, m, pair = C.degenerate_case(name)
        for linear in ("eigh", "svd"):
            F, q, ns, st = T.two_view(pt_ptr, cam, xy, m, [pair], linear)
            assert st[0] == 2 and np.isnan(F).all() and np.isnan(q).all() and ns[0] == len(pt_ptr) - 1


def test_limit_cases_have_the_stated_sizes_and_statuses():
    """The premises of tests/test_gpu_twoview_limits.py that need no device, and the statuses the reference defines for a
    pair without shared points and for coincident image points (an infinite Hartley scale), by either linear route."""
    pt_ptr, cam, xy, m, six = C.case("16641x3")
    assert -(-(len(pt_ptr) - 1) // C.TV_CHUNK) == 66 and [tuple(p) for p in six] == [(0, 1), (0, 2), (1, 2), (1, 0), (2, 0), (2, 1)]
    assert C.pair_tile(16641, 5700) == 5648 and C.pair_tile(300, 65600) == 65535 and C.pair_tile(300, 30) == 30
    assert len(C.cycled(six, 5700)) == 5700 and (C.cycled(six, 5700)[5694:] == six).all()
    pt_ptr, cam, xy, m = C.no_shared_case()
    F, q, ns, st = T.two_view(pt_ptr, cam, xy, m, [(0, 8), (8, 3)])
    assert ns.tolist() == [0, 0] and st.tolist() == [1, 1] and np.isnan(F).all() and np.isnan(q).all()
    import _init_cases as IC

    pt_ptr, cam, xy0, m, pairs = C.case("300x8")
    hit = (pairs == IC.COINCIDENT_CAMERA).any(axis=1)
    for kind in sorted(IC.COINCIDENT_POINTS):
        for linear in ("eigh", "svd"):
            F, q, ns, st = T.two_view(pt_ptr, cam, IC.coincident_xy(kind), m, pairs, linear)
            np.testing.assert_array_equal(st, np.where(hit, 2, 0))
            np.testing.assert_array_equal(ns, C.reference("300x8")[2])
            assert np.isnan(F[hit]).all() and np.isnan(q[hit]).all()
            if linear == "eigh":
                np.testing.assert_array_equal(F[~hit], C.reference("300x8")[0][~hit])


def test_host_helpers_of_the_product_agree_with_the_reference():
    sc = C.scene("300x8")
    po, co = np.arange(300) % 3 > 0, np.arange(8) != 4
    for a, b in zip(restrict_observations(sc.pt_ptr, sc.cam_idx, sc.xy, po, co), T.restrict(sc.pt_ptr, sc.cam_idx, sc.xy, po, co)):
        np.testing.assert_array_equal(a, b)
    E = C.true_essential(C.scene("noise_free"), 0, 1)
    for (Ra, ta), (Rb, tb) in zip(pose_candidates(E), T.pose_candidates(E)):
        np.testing.assert_array_equal(Ra, Rb)
        np.testing.assert_array_equal(ta, tb)
        assert abs(np.linalg.det(Ra) - 1.0) < 1e-14 and abs(np.linalg.norm(ta) - 1.0) < 1e-14
    # pose_for_intrinsics: with P's own intrinsics it returns P's own pose; with another focal length the centre moves
    # along the ray of c so that c keeps its image and f / depth
    import _init_ref as ref

    K = engine_intrinsics(sc.init_K)
    P = ref.camera_matrices(K, sc.R_gt, sc.t_gt)[3]
    c = np.array([0.1, -0.2, 0.05])
    R, t = pose_for_intrinsics(P, K[3], c)
    np.testing.assert_allclose(R, sc.R_gt[3], rtol=0, atol=1e-13)
    np.testing.assert_allclose(t, sc.t_gt[3], rtol=0, atol=1e-12)
    K2 = K[3].copy()
    K2[0, 0] = K2[1, 1] = 1.05 * K[3, 0, 0]
    R2, t2 = pose_for_intrinsics(P, K2, c)
    for got, want in zip((R2, t2), T.pose_for_intrinsics(P, K2, c)):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
    y, y2 = sc.R_gt[3].T @ (c - sc.t_gt[3]), R2.T @ (c - t2)
    np.testing.assert_allclose(y2[:2] / y2[2] * 1.05, y[:2] / y[2], rtol=0, atol=1e-13)
    np.testing.assert_allclose(y2[2], 1.05 * y[2], rtol=1e-13)


def test_reference_bootstrap_registers_everything():
    """The route of the issue on make_scene(300, 8, 0.5): 8 cameras, 300 points, an RMS reprojection residual of the order of
    the noise (1e-3) before any BA."""
    sc = C.scene("300x8")
    K = engine_intrinsics(sc.init_K)
    R, t, X, info = T.bootstrap(sc.pt_ptr, sc.cam_idx, sc.xy, K)
    assert info["camera_ok"].all() and info["point_ok"].all() and sorted(info["order"]) == list(range(8))
    rms = T.rms_reprojection(K, R, t, X, sc.pt_ptr, sc.cam_idx, sc.xy)
    print(f"start pair {info['start_pair']}, order {info['order']}, axis {info['axis']}, RMS residual {rms:.3e}")
    assert rms < 5e-3  # measured 1.9e-3; the noise is 1e-3 and K is off by 1 %
    np.testing.assert_allclose(R[0], np.eye(3), rtol=0, atol=1e-15)
    assert np.abs(t[0]).max() < 1e-15 and abs(np.linalg.norm(t[1]) - 1.0) < 1e-14
    g = 0 if info["axis"] == "x-right_z-forward" else 1
    assert abs(t[1, g]) == np.abs(t[1, :2]).max()
    # a camera with fewer than min_points observations is left out; camera 0 or 1 left out is an error
    pt_ptr, cam, xy = C.short_camera_scene(5)
    R, t, X, info = T.bootstrap(pt_ptr, cam, xy, K)
    assert info["camera_ok"].tolist() == [True] * 5 + [False] + [True] * 2 and np.isnan(R[5]).all()
    with pytest.raises(ValueError, match="camera 1"):
        T.bootstrap(*C.short_camera_scene(1), K)


def test_library_exports_the_two_view_entry_points():
    """The test that fails before this feature: the symbols of include/mvba.h exist in libmvba.so, with prototypes bound."""
    assert "mvba_covisibility" in _mvba.SIGNATURES and "mvba_two_view" in _mvba.SIGNATURES
    if not os.path.exists(_mvba.LIB_PATH):
        pytest.skip("libmvba.so is not built")
    lib = ctypes.CDLL(_mvba.LIB_PATH)
    for name in ("mvba_covisibility", "mvba_two_view"):
        assert hasattr(lib, name), name
    # argument errors come before any device work: they need no GPU
    lib = _mvba.load_library()
    i32, i64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    pt_ptr, cam, xy, m, _ = C.case("300x8")
    F = np.empty((1, 9))

    def call(pair, n_pairs=1):
        pairs = np.array(pair, np.int32)
        rc = lib.mvba_two_view(300, m, pt_ptr.ctypes.data_as(i64), cam.ctypes.data_as(i32), _mvba._ptr(xy), len(cam),
                               pairs.ctypes.data_as(i32), n_pairs, _mvba._ptr(F), None, None, None, None, -1)
        return rc, lib.mvba_last_error().decode()

    rc, msg = call((3, 3))
    assert rc == _mvba.MVBA_ERR_BADARG and "(3, 3)" in msg
    rc, msg = call((2, 8))
    assert rc == _mvba.MVBA_ERR_BADARG and "(2, 8)" in msg and "n_images = 8" in msg
    rc, msg = call((0, 1), n_pairs=-4)
    assert rc == _mvba.MVBA_ERR_BADARG and "n_pairs = -4" in msg
    assert lib.mvba_covisibility(300, m, pt_ptr.ctypes.data_as(i64), cam.ctypes.data_as(i32), len(cam), None, None, -1) == _mvba.MVBA_ERR_BADARG


def test_two_view_fails_loudly_without_gpu():
    if os.path.exists(_mvba.LIB_PATH) and _mvba.device_count() > 0:
        pytest.skip("a device is visible")
    pt_ptr, cam, xy, m, pairs = C.case("300x8")
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        _mvba.two_view(pt_ptr, cam, xy, m, pairs)
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        _mvba.covisibility(pt_ptr, cam, m)
