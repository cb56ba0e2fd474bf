"""Robust triangulation on the device: mvba_triangulate_robust against the NumPy restatement of
tests/_tri_ransac_ref.py -- count tables, best hypotheses, inlier counts, statuses and the inlier bytes EXACTLY
(tests/test_tri_ransac_cpu.py asserts the premises under which that may be asked), X and quality within 100 x the
host-versus-host difference of the very case (tests/_tri_ransac_cases.py) --, its structure (grid stride, refit counts, status
shapes, bad arguments, two calls), and bootstrap with ``triangulate_threshold`` on tracks contaminated in every camera.

X and the three quality figures are compared absolutely, within one margin: coordinates, depths and angles are of order 1, and
a change dX of a point moves its reprojections by about f |dX| / depth in the units of xy -- which is why the "pixels" case's
own host-versus-host figure is that of its RMS residual, 1.3e-13 pixels."""
import numpy as np
import pytest

import _init_cases as IC
import _tri_ransac_cases as TC
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster
from lib.initialization import bootstrap, robust_triangulate_points, triangulate_points

pytestmark = pytest.mark.gpu

EXACT = ("hyp_count", "best", "n_inliers", "status", "inlier")
KEYS = ("X", "quality") + EXACT


def _run(K, R, t, pt_ptr, cam, xy, thr, H, n_refine=2, n_refit=2, seed=TC.SEED, counts=True):
    return _mvba.triangulate_robust(K, R, t, pt_ptr, cam, xy, thr, n_hypotheses=H, seed=seed, n_refine=n_refine, n_refit=n_refit,
                                    return_counts=counts)


def _assert_exact(got, want, what):
    for key in EXACT:
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")


def _assert_close(got, want, margin, what):
    """X and quality within ``margin`` of the reference's -- of ONE of its outcomes where a Gauss-Newton step of the last refit
    changes the cost by less than the cost's own rounding (tests/_tri_ransac_ref.py: refine_candidates; the reference lists
    them without knowing the device's arithmetic)."""
    ok = want["status"] == 0
    bad = ~ok
    assert np.isnan(got["X"][bad]).all() and np.isnan(got["quality"][bad]).all()
    if not ok.any():
        return
    dX = np.abs(got["X"][ok][:, None, :] - want["alt_X"][ok]).max(axis=2)  # (points, outcomes), NaN where there is none
    dq = np.abs(got["quality"][ok][:, None, :] - want["alt_quality"][ok])
    worst = np.where(np.isnan(dX), np.inf, np.fmax(dX, dq.max(axis=2)))
    pick, rows = worst.argmin(axis=1), np.arange(int(ok.sum()))
    d, dq = dX[rows, pick].max(), dq[rows, pick].max(axis=0)
    print(f"{what}: max |dX| {d:.3e}, RMS {dq[0]:.3e}, depth {dq[1]:.3e}, angle {dq[2]:.3e} (margin {margin:.1e}); "
          f"{(pick > 0).sum()} of the {(want['n_ties'][ok] > 0).sum()} points with a tied step took its other side")
    assert d <= margin and (dq <= margin).all()


@pytest.mark.parametrize("name", sorted(TC.PARITY))
def test_parity(name):
    K, R, t, pt_ptr, cam, xy, thr, H, _ = TC.case(name)
    margin = TC.MARGIN * TC.TRI_RANSAC_HOST_DIFF[name]
    got, want = _run(K, R, t, pt_ptr, cam, xy, thr, H), TC.reference(name)
    _assert_exact(got, want, name)
    _assert_close(got, want, margin, name)
    assert set(got["timings_ms"]) == {"upload", "score", "refit", "download"} and got["timings_ms"]["score"] > 0 and got["timings_ms"]["refit"] > 0
    got0, want0 = _run(K, R, t, pt_ptr, cam, xy, thr, H, n_refine=0), TC.reference(name, 0, 2)  # the linear refit alone
    _assert_exact(got0, want0, name + ", n_refine = 0")
    _assert_close(got0, want0, margin, name + ", n_refine = 0")
    if name in ("300x8", "pixels"):  # the public call
        X, info = robust_triangulate_points(pt_ptr, cam, xy, K, R, t, thr, n_hypotheses=H, seed=TC.SEED)
        assert X.tobytes() == got["X"].tobytes() and np.array_equal(info["inlier"], got["inlier"]) and "X" not in info
        np.testing.assert_array_equal(info["confidence"], (want["status"] == 0).astype(float))  # (every pair tried)
    if name == "65x70_h17":  # sampled: 1 - (1 - w^2)^H
        _, info = robust_triangulate_points(pt_ptr, cam, xy, K, R, t, thr, n_hypotheses=H, seed=TC.SEED)
        w = want["n_inliers"] / 70.0
        np.testing.assert_allclose(info["confidence"], np.where(want["status"] == 0, 1.0 - (1.0 - w ** 2) ** H, 0.0), rtol=1e-12)
    if name == "300x8":  # without refits: the best midpoint itself
        m0, w0 = _run(K, R, t, pt_ptr, cam, xy, thr, H, n_refit=0), TC.reference(name, 2, 0)
        _assert_exact(m0, w0, name + ", n_refit = 0")
        _assert_close(m0, w0, TC.MARGIN * TC.MIDPOINT_HOST_DIFF["300x8"], name + ", n_refit = 0")
        ok = m0["status"] == 0
        np.testing.assert_array_equal(m0["n_inliers"][ok], m0["hyp_count"].max(axis=1)[ok])
    if name == "dense":  # the dense grid and the list form are one computation
        p, c = IC.ref.dense_list(xy.shape[0], len(K))
        listed = _run(K, R, t, p, c, np.asarray(xy).reshape(-1, 2), thr, H)
        for key in KEYS:
            assert listed[key].tobytes() == got[key].tobytes(), key


def test_robust_against_plain_on_clean_and_contaminated_tracks():
    """What the kernel is for: on "300x8" with 20 % replaced, every point with three clean observations gets exactly its clean
    set and lands within 0.03 of the truth, where the plain kernel on the same list is off by more than 1."""
    K, R, t, pt_ptr, cam, xy, thr, H, hit = TC.case("300x8")
    ge3, clean = TC.clean_sets("300x8")
    pt = np.repeat(np.arange(300), np.diff(pt_ptr))
    got = _run(K, R, t, pt_ptr, cam, xy, thr, H, counts=False)
    assert "hyp_count" not in got and (got["status"][ge3] == 0).all()
    np.testing.assert_array_equal(got["inlier"][ge3[pt]], clean[ge3[pt]])
    X_gt = IC.tri_scene("300x8").X_gt
    plain = triangulate_points(pt_ptr, cam, xy, K, R, t)[0]
    e, ep = np.linalg.norm(got["X"][ge3] - X_gt[ge3], axis=1), np.linalg.norm(plain[ge3] - X_gt[ge3], axis=1)
    print(f"robust max {e.max():.3g}, plain max {np.nanmax(ep):.3g}")
    assert e.max() < 0.03 and np.nanmax(ep) > 1.0


@pytest.mark.parametrize("n_refit", TC.REFIT_COUNTS)
def test_refit_counts(n_refit):
    K, R, t, pt_ptr, cam, xy, _, H, _ = TC.case("300x8")
    got, want = _run(K, R, t, pt_ptr, cam, xy, TC.REFIT_THRESHOLD, H, n_refit=n_refit), TC.refit_reference(n_refit)
    _assert_exact(got, want, f"n_refit = {n_refit}")
    _assert_close(got, want, TC.MARGIN * (TC.MIDPOINT_HOST_DIFF["refit"] if n_refit == 0 else TC.TRI_RANSAC_HOST_DIFF["300x8"]), f"n_refit = {n_refit}")


def test_status_shapes():
    K, R, t, pt_ptr, cam, xy = TC.status_case()
    got, want = _run(K, R, t, pt_ptr, cam, xy, TC.THRESHOLD, TC.STATUS_HYP), TC.status_reference()
    _assert_exact(got, want, "status shapes")
    _assert_close(got, want, TC.MARGIN * TC.STATUS_HOST_DIFF, "status shapes")
    st = got["status"]
    assert st[3] == 1 and st[7] == 2 and st[11] == 2 and st[TC.ALL_REPLACED] == 4 and st[TC.ONE_OF_THREE] == 4
    assert st[TC.TWO_VIEWS] == 0 and got["n_inliers"][TC.TWO_VIEWS] == 2
    bad = st != 0
    pt = np.repeat(np.arange(40), np.diff(pt_ptr))
    assert (got["n_inliers"][bad] == 0).all() and not got["inlier"][bad[pt]].any()
    assert (got["best"][[3, 7, 11]] == -1).all() and (got["best"][[TC.ALL_REPLACED, TC.ONE_OF_THREE]] >= 0).all()


def test_grid_stride_every_tile_is_bitwise_the_first():
    """The "300x8" list 1754 times along the point axis: 526 200 points, 32 888 groups of k_tri_score against a grid of 2048
    workgroups of 16, and k_tri_refit past its 2048 x 256 threads.  Every point is exhaustive (at most 28 pairs in 64), so its
    result does not depend on its index: every tile is bitwise the first, and the first is the reference's."""
    reps, pt_ptr, cam, _ = IC.tiled_scene()
    K, R, t, _, _, xy, thr, H, _ = TC.case("300x8")
    assert len(pt_ptr) - 1 > IC.GRID_CAP
    got = _run(K, R, t, pt_ptr, cam, np.tile(xy, (reps, 1)), thr, H, counts=False)
    n_obs = len(xy)
    for key in ("X", "quality", "status", "n_inliers", "best"):
        tiles = got[key].reshape((reps, 300) + got[key].shape[1:])
        assert all(tiles[r].tobytes() == tiles[0].tobytes() for r in range(1, reps)), key
    assert (got["inlier"].reshape(reps, n_obs) == got["inlier"][:n_obs]).all()
    first = {key: got[key][:300] for key in ("X", "quality", "status", "n_inliers", "best")}
    first["inlier"] = got["inlier"][:n_obs]
    want = TC.reference("300x8")
    for key in ("best", "n_inliers", "status", "inlier"):
        np.testing.assert_array_equal(first[key], want[key], err_msg=key)
    _assert_close(first, want, TC.MARGIN * TC.TRI_RANSAC_HOST_DIFF["300x8"], "first tile")


def test_two_calls_are_bitwise_equal_and_the_seed_moves_the_sample():
    for name in ("300x8", "65x70_h17", "300x1704"):
        K, R, t, pt_ptr, cam, xy, thr, H, _ = TC.case(name)
        a, b = _run(K, R, t, pt_ptr, cam, xy, thr, H), _run(K, R, t, pt_ptr, cam, xy, thr, H)
        for key in KEYS:
            assert a[key].tobytes() == b[key].tobytes(), (name, key)
        c = _run(K, R, t, pt_ptr, cam, xy, thr, H, seed=TC.SEED + 1)
        if name == "300x8":  # every pair tried: the seed is not used
            assert all(a[key].tobytes() == c[key].tobytes() for key in KEYS)
        else:
            assert not np.array_equal(a["hyp_count"], c["hyp_count"])


def test_bad_arguments():
    K, R, t, pt_ptr, cam, xy, thr, _, _ = TC.case("300x8")
    for kw, text in (({"threshold": -0.01}, "threshold = -0.01"), ({"threshold": 0.0}, "threshold = 0.0"), ({"threshold": np.inf}, "threshold = inf"),
                     ({"n_hypotheses": 0}, "n_hypotheses = 0"), ({"n_hypotheses": 4097}, "n_hypotheses = 4097"), ({"n_refit": -1}, "n_refit = -1"),
                     ({"n_refit": 17}, "n_refit = 17"), ({"n_refine": -1}, "n_refine = -1")):
        args = {"threshold": thr, "n_hypotheses": 16, "n_refit": 2, "n_refine": 2}
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            _mvba.triangulate_robust(K, R, t, pt_ptr, cam, xy, args.pop("threshold"), **args)
    bad_cam = cam.copy()
    bad_cam[7] = 8
    with pytest.raises(ValueError, match="cam_idx out of range"):
        _mvba.triangulate_robust(K, R, t, pt_ptr, bad_cam, xy, thr)
    lib = _mvba.load_library()  # a null X: MVBA_ERR_BADARG before anything is launched
    import ctypes as C
    Kc, Rc, tc, xyc = (np.ascontiguousarray(v) for v in (K, R, t, xy))
    rc = lib.mvba_triangulate_robust(_mvba._ptr(Kc), _mvba._ptr(Rc), _mvba._ptr(tc), 8, 300, pt_ptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                     cam.ctypes.data_as(C.POINTER(C.c_int32)), _mvba._ptr(xyc), len(cam), thr, 16, 1, 2, 2, None, None, None, None,
                                     None, None, None, None, -1)
    assert rc == _mvba.MVBA_ERR_BADARG and "null argument: X" in lib.mvba_last_error().decode()


def _huber_cost(n, pt_ptr, cam, xy, X, K, R, t, delta):
    eng = _mvba.HipEngine(n, 8, pt_ptr, cam, xy, 1.0, "x-up_z-forward", loss="huber", loss_scale=delta)
    eng.set_params(X, K[:, 0, 0], K[:, :2, 2], t, R)
    E = eng.cost()
    eng.close()
    return E


def _inlier_list(pt_ptr, cam, xy, use, point_ok):
    """The list of the observations ``use`` of the points ``point_ok``, points renumbered: (pt_ptr, cam_idx, xy, point ids)."""
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    keep = use & point_ok[pt]
    pid = np.nonzero(point_ok)[0]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(pt[keep], minlength=len(pt_ptr) - 1)[pid])]).astype(np.int64)
    return ptr, cam[keep], xy[keep], pid


def test_bootstrap_with_robust_triangulation_then_robust_bundle_adjustment():
    """20 % of the observations of ALL cameras replaced, ransac_threshold and resect_threshold set.  With triangulate_threshold
    the driver is the reference's: 8 cameras, 205 points, no point triangulated from a replaced observation if it has three clean
    ones, 7 points farther than 0.1 from the truth; Huber BA over the observations the points were triangulated from ends
    below the cost of the ground truth on that list.  The same call without it keeps all 300 points and 88 of them are farther
    than 0.1 from the truth (the figures of the CPU reference runs: tests/test_tri_ransac_cpu.py)."""
    sc, xy, hit = TC.bootstrap_case()
    kw = dict(start_pair=(0, 1), ransac_threshold=TC.BOOT_RANSAC_THRESHOLD, resect_threshold=TC.THRESHOLD, n_hypotheses=TC.BOOT_HYP, seed=TC.SEED)
    K, R, t, X, info = bootstrap(sc.pt_ptr, sc.cam_idx, xy, sc.init_K, triangulate_threshold=TC.THRESHOLD, **kw)
    Rr, tr, Xr, ir = TC.reference_bootstrap(True)
    assert info["order"] == ir["order"] and info["camera_ok"].all() and len(info["order"]) == 8
    for key in ("camera_ok", "point_ok", "obs_ok", "inlier", "tri_inlier"):
        np.testing.assert_array_equal(info[key], ir[key], err_msg=key)
    ok = info["point_ok"]
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    ge3 = np.bincount(pt[~hit], minlength=sc.n_points) >= 3
    assert not (info["tri_inlier"] & hit & ge3[pt]).any()
    dX = np.nanmin(np.abs(X[ok][:, None, :] - ir["alt_X"][ok]).max(axis=2), axis=1).max()  # (either side of a tied Gauss-Newton step)
    d = max(np.abs(R - Rr).max(), np.abs(t - tr).max(), dX)
    far = int((TC.point_error(sc, X, ok) > TC.BOOT_FAR).sum())
    print(f"robust: {ok.sum()} points, {far} far, |d| to the reference {d:.2e} (margin {TC.MARGIN * TC.BOOT_HOST_DIFF:.1e})")
    assert d <= TC.MARGIN * TC.BOOT_HOST_DIFF
    assert (int(ok.sum()), far) == TC.BOOT_REFERENCE_FIGURES[:2]
    ptr, cam, z, pid = _inlier_list(sc.pt_ptr, sc.cam_idx, xy, info["tri_inlier"], ok)
    ba = BundleAdjuster.from_observations(len(pid), 8, ptr, cam, z, X[pid], K, R, t, axis=info["axis"], loss="huber", loss_scale=TC.BOOT_DELTA)
    E0 = ba._engine.cost()
    ba.optimize()
    E, E_gt = ba._engine.cost(), _huber_cost(len(pid), ptr, cam, z, sc.X_gt[pid], sc.K_gt, sc.R_gt, sc.t_gt, TC.BOOT_DELTA)
    print(f"huber cost {E0:.4e} -> {E:.4e}, ground truth {E_gt:.4e}")
    assert E < E_gt
    # the same call without triangulate_threshold: every triangulation is the plain one, and the outliers move the points
    _, _, _, Xp, ip = bootstrap(sc.pt_ptr, sc.cam_idx, xy, sc.init_K, **kw)
    assert "tri_inlier" not in ip and ip["camera_ok"].all()
    far_p = int((TC.point_error(sc, Xp, ip["point_ok"]) > TC.BOOT_FAR).sum())
    print(f"plain: {ip['point_ok'].sum()} points, {far_p} far")
    assert (int(ip["point_ok"].sum()), far_p) == TC.BOOT_REFERENCE_FIGURES[2:]
    assert far_p >= TC.BOOT_CONTRAST * max(far, 1)
