"""Initial estimates, the part that needs no GPU: the NumPy reference of tests/_init_ref.py recovers the
ground truth of a noise-free scene, its status rules hold on constructed cases, the host-versus-host differences that set
the GPU parity margins are what tests/_init_cases.py records, decompose_projection round-trips, and the product path
fails loudly without a device."""
import numpy as np
import pytest

import _init_cases as C
import _init_ref as ref
from lib.bundle_adjustment import BundleAdjuster, dense_to_observations
from lib.initialization import decompose_projection, engine_intrinsics
from lib.synthetic import make_cameras, make_scene


def test_reference_recovers_a_noise_free_scene():
    sc = make_scene(300, 8, vis_p=0.5, noise=0.0, project="numpy")
    for n_refine in (0, 2):
        X, q, st = ref.triangulate(sc.K_gt, sc.R_gt, sc.t_gt, sc.pt_ptr, sc.cam_idx, sc.xy, n_refine)
        assert (st == 0).all()
        err = np.abs(X - sc.X_gt).max()
        print(f"triangulate n_refine={n_refine}: max |X - X_gt| = {err:.3e}, max RMS residual = {q[:, 0].max():.3e}")
        assert err < 1e-12  # measured 2.6e-15 (n_refine 0), 7.8e-16 (2)
        assert q[:, 0].max() < 1e-13 and q[:, 1].min() > 0 and (q[:, 2] > 0).all() and (q[:, 2] < np.pi).all()
    P, q, st = ref.resect(sc.X_gt, sc.pt_ptr, sc.cam_idx, sc.xy, 8)
    P_gt = ref.camera_matrices(sc.K_gt, sc.R_gt, sc.t_gt)
    P_gt = P_gt / np.linalg.norm(P_gt[:, 2, :3], axis=1)[:, None, None]
    err = np.abs(P.reshape(8, 3, 4) - P_gt).max()
    print(f"resect: max |P - P_gt| = {err:.3e}, max ratio = {q[:, 1].max():.3e}")
    assert (st == 0).all() and err < 1e-11  # measured 1.2e-14
    assert np.abs(q[:, 1]).max() < 1e-12 and q[:, 0].max() < 1e-12


def test_decompose_projection_round_trips_make_cameras():
    K, R, t, K0, R0, t0 = make_cameras(9)
    K0[:, :2, 2] = np.random.default_rng(0).normal(0, 0.05, (9, 2))
    for Kx, Rx, tx in ((K, R, t), (K0, R0, t0)):  # f0 = 1: P = K [R^T | -R^T t]
        P = ref.camera_matrices(Kx, Rx, tx)
        for scale in (1.0, -2.5):  # (a camera matrix is defined up to scale and sign)
            K2, R2, t2 = decompose_projection(scale * P, 1.0)
            np.testing.assert_allclose(K2, Kx, rtol=0, atol=1e-12)
            np.testing.assert_allclose(R2, Rx, rtol=0, atol=1e-12)
            np.testing.assert_allclose(t2, tx, rtol=0, atol=1e-11)
    K1, R1, t1 = decompose_projection(ref.camera_matrices(K, R, t)[3])
    assert K1.shape == (3, 3) and np.allclose(R1, R[3]) and np.allclose(t1, t[3])


def test_pixel_units_f0_is_not_part_of_the_projection_to_raw_xy():
    """f0 != 1: the adjuster's init_K = [[f,0,u],[0,f,v],[0,0,f0]] projects to x / f0, its xy are raw pixels.  The matrix that
    belongs to raw xy has K[2, 2] = 1 (what mvba_triangulate_state forms, lib.initialization.engine_intrinsics); the one with
    f0 in it is wrong by thousands and raises nothing, which is why the GPU tests check this case.  decompose_projection
    returns the adjuster's init_K from a matrix that projects to raw pixels."""
    sc, xy_px, K, K_raw = C.pixel_scene(noise_free=True)
    np.testing.assert_array_equal(engine_intrinsics(K), K_raw)
    X, q, st = ref.triangulate(K_raw, sc.R_gt, sc.t_gt, sc.pt_ptr, sc.cam_idx, xy_px, 2)
    assert (st == 0).all() and np.abs(X - sc.X_gt).max() < 1e-12 and q[:, 0].max() < 1e-10  # (RMS in pixels)
    Xw, _, stw = ref.triangulate(K, sc.R_gt, sc.t_gt, sc.pt_ptr, sc.cam_idx, xy_px, 2)
    assert np.nanmax(np.abs(Xw - sc.X_gt)) > 1.0  # the trap
    # the engine's own residual (oracle) at the triangulated points, with the adjuster's f, u and f0 = 600, is zero
    from oracle import ba_oracle as O

    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    e = O.residuals(X, K[:, 0, 0], K[:, :2, 2], sc.t_gt, sc.R_gt, C.PIXEL_F0, pt, sc.cam_idx, xy_px)
    assert np.abs(e).max() < 1e-13
    K2, R2, t2 = decompose_projection(3.0 * ref.camera_matrices(K_raw, sc.R_gt, sc.t_gt), C.PIXEL_F0)
    np.testing.assert_allclose(K2, K, rtol=0, atol=1e-9)
    np.testing.assert_allclose(R2, sc.R_gt, rtol=0, atol=1e-12)
    np.testing.assert_allclose(t2, sc.t_gt, rtol=0, atol=1e-11)


@pytest.mark.parametrize("name", sorted(C.TRI_HOST_DIFF))
def test_triangulation_host_versus_host_difference(name):
    """eigh(M) against the SVD of the stacked rows: the figure the GPU parity margin is 100 x of."""
    a, b = C.tri_reference(name, 0), C.tri_reference(name, 0, "svd")
    assert (a[2] == 0).all() and (b[2] == 0).all()  # (every point has degree >= 2 and parallax: all must triangulate)
    d = np.abs(a[0] - b[0]).max()
    print(f"{name}: eigh vs SVD max |dX| = {d:.3e} (recorded {C.TRI_HOST_DIFF[name]:.1e})")
    assert 0.5 * C.TRI_HOST_DIFF[name] <= d <= C.TRI_HOST_DIFF[name]
    a2, b2 = C.tri_reference(name, 2), C.tri_reference(name, 2, "svd")
    assert np.abs(a2[0] - b2[0]).max() <= C.TRI_HOST_DIFF[name]  # (measured 4.4e-16 at most: the refinement converges)


def test_issue_scene_has_the_stated_conditioning():
    """make_scene(300, 8, vis_p=0.5): every degree >= 3 and the smallest lambda_2 / lambda_4 is 0.013."""
    sc = C.tri_scene("300x8")
    assert np.diff(sc.pt_ptr).min() >= 3 and sc.n_points % 64 != 0
    P = ref.camera_matrices(sc.init_K, sc.init_R, sc.init_t)
    lo = 1.0
    for a in range(sc.n_points):
        o = slice(sc.pt_ptr[a], sc.pt_ptr[a + 1])
        rows = ref.point_rows(P, sc.cam_idx[o], sc.xy[o])
        w = np.linalg.eigvalsh(rows.T @ rows)
        lo = min(lo, w[1] / w[3])
    assert 0.005 < lo < 0.03, lo


@pytest.mark.parametrize("name", sorted(C.RESECT_HOST_DIFF))
def test_resection_host_versus_host_difference(name):
    a, b = C.resect_reference(name), C.resect_reference(name, "svd")
    assert (a[2] == b[2]).all() and (a[2] == C.resect_case(name)[5]).all()
    d = np.nanmax(np.abs(a[0] - b[0]))
    print(f"{name}: eigh vs SVD max |dP| = {d:.3e} (recorded {C.RESECT_HOST_DIFF[name]:.1e})")
    assert 0.5 * C.RESECT_HOST_DIFF[name] <= d <= C.RESECT_HOST_DIFF[name]


def test_status_rules_on_constructed_cases():
    K, R, t, pt_ptr, cam, xy, expect, X_gt = C.status_case()
    for n_refine in (0, 2):
        X, q, st = ref.triangulate(K, R, t, pt_ptr, cam, xy, n_refine)
        np.testing.assert_array_equal(st, expect)
        bad = expect != 0
        assert np.isnan(X[bad]).all() and np.isnan(q[bad]).all()
        np.testing.assert_allclose(X[~bad], X_gt[~bad], rtol=0, atol=1e-12)  # (the neighbours are unaffected)
    X, pt_ptr, cam, xy, m, expect = C.resect_case("six")
    P, q, st = ref.resect(X, pt_ptr, cam, xy, m)
    np.testing.assert_array_equal(st, expect)
    assert np.isnan(P[2]).all() and np.isfinite(P[[0, 1, 3]]).all()
    X, pt_ptr, cam, xy, m, expect = C.resect_case("coplanar")
    P, q, st = ref.resect(X, pt_ptr, cam, xy, m)
    np.testing.assert_array_equal(st, expect)
    assert np.isnan(P).all()
    # point_ok: the masked points do not count (a camera drops below 6 usable observations)
    X, pt_ptr, cam, xy, m, _ = C.resect_case("six")
    ok = np.ones(60, bool)
    ok[0] = False
    assert ref.resect(X, pt_ptr, cam, xy, m, point_ok=ok)[2].tolist() == [0, 1, 1, 0]
    Xn = X.copy()
    Xn[0] = np.nan  # (the default mask: the points whose X is finite)
    assert ref.resect(Xn, pt_ptr, cam, xy, m)[2].tolist() == [0, 1, 1, 0]


def test_limit_scenes_have_the_stated_properties():
    """The premises of tests/test_gpu_init_limits.py that need no device."""
    reps, pt_ptr, cam, xy = C.tiled_scene()
    sc = C.tri_scene("300x8")
    assert reps == 1754 and len(pt_ptr) - 1 == 526200 > C.GRID_CAP == 524288
    np.testing.assert_array_equal(np.diff(pt_ptr).reshape(reps, 300), np.tile(np.diff(sc.pt_ptr), (reps, 1)))
    assert pt_ptr[-1] == len(cam) == len(xy) == reps * sc.n_obs and np.array_equal(cam[-sc.n_obs:], sc.cam_idx)
    for name, m, rows in (("300x683", 683, [682]), ("300x1704", 1704, [682, 683, 1703])):
        sc = C.tri_scene(name)
        assert sc.n_images == m and 12 * 8 * m > 65536 and all((sc.cam_idx == r).any() for r in rows)
        assert (C.tri_reference(name, 0)[2] == 0).all() and (C.tri_reference(name, 2)[2] == 0).all()  # 300 of 300
    assert 12 * 8 * 1704 == 163584 <= 160 * 1024 - 256 < 12 * 8 * 1705
    X, pt_ptr, cam, xy, m, expect = C.resect_case("900x300")
    st = C.resect_reference("900x300")[2]
    print(f"900x300: {int((st == 1).sum())} cameras with fewer than 6 observations, {int((st == 0).sum())} of {m} resected")
    assert m > 256 and (st == expect).all() and (st == 0).sum() >= 0.95 * m
    X, pt_ptr, cam, xy, m, _ = C.resect_case("edges")
    assert np.bincount(cam).tolist() == [257, 256, 255]


def test_reference_defines_the_degenerate_inputs():
    """The inputs of tests/test_gpu_init_limits.py that make a Hartley scale infinite or leave a camera without
    observations: the reference gives them the statuses of include/mvba.h, by either linear route."""
    K, R, t, pt_ptr, cam, xy, expect = C.duplicate_observation_case()
    assert cam[pt_ptr[5]:pt_ptr[6]].tolist() == [2, 2] and (xy[pt_ptr[5]] == xy[pt_ptr[5] + 1]).all()
    for linear in ("eigh", "svd"):
        X, q, st = ref.triangulate(K, R, t, pt_ptr, cam, xy, 2, linear=linear)
        np.testing.assert_array_equal(st, expect)
        assert st[5] == 2 and np.isnan(X[5]).all() and np.isnan(q[5]).all()
    X, pt_ptr, cam, xy0, m, _ = C.resect_case("300x8")
    P0 = ref.resect(X, pt_ptr, cam, xy0, m)[0]
    for kind in sorted(C.COINCIDENT_POINTS):
        xy = C.coincident_xy(kind)
        assert (xy[cam == C.COINCIDENT_CAMERA] == C.COINCIDENT_POINTS[kind]).all() and (xy[cam != C.COINCIDENT_CAMERA] == xy0[cam != C.COINCIDENT_CAMERA]).all()
        for linear in ("eigh", "svd"):
            P, q, st = ref.resect(X, pt_ptr, cam, xy, m, linear=linear)
            assert st.tolist() == [0, 0, 0, 2, 0, 0, 0, 0] and np.isnan(P[3]).all() and np.isnan(q[3, 0])
            if kind == "exact":  # the scale is sqrt(2) / sqrt(0): the rows are NaN, there is no eigenvalue ratio
                assert np.isnan(q[3, 1])
            if linear == "eigh":
                np.testing.assert_array_equal(P[st == 0], P0[st == 0])
    X, pt_ptr, cam, xy, m, kept = C.empty_camera_case()
    P, q, st = ref.resect(X, pt_ptr, cam, xy, m)
    assert np.nonzero(st == 1)[0].tolist() == list(C.EMPTY_CAMERAS) and np.isnan(P[st == 1]).all() and np.isnan(q[st == 1]).all()
    np.testing.assert_array_equal(P[kept], P0)
    for kw in ({"point_ok": np.zeros(len(X), bool)}, {}):
        P, q, st = ref.resect(X if kw else np.full_like(X, np.nan), pt_ptr, cam, xy, m, **kw)
        assert (st == 1).all() and np.isnan(P).all() and np.isnan(q).all()


def test_init_X_none_fails_loudly_without_gpu(golden):
    """from_observations(init_X=None) on a box without a GPU fails as the product path does today (tests/test_host_cpu.py)."""
    from lib import _mvba

    d = golden("visibility_300x12")
    pt_ptr, cam_idx, xy = dense_to_observations(d["x"], d["vis"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BundleAdjuster.from_observations(300, 12, pt_ptr, cam_idx, xy, None, d["init_K"], d["init_R"], d["init_t"], axis="x-up_z-forward")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BundleAdjuster(d["x"], None, d["init_K"], d["init_R"], d["init_t"], visibility_index=d["vis"], axis="x-up_z-forward")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _mvba.triangulate(d["init_K"], d["init_R"], d["init_t"], pt_ptr, cam_idx, xy)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _mvba.resect(d["init_X"], pt_ptr, cam_idx, xy, 12)
