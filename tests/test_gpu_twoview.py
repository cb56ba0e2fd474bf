"""The two-view start on the device: mvba_covisibility and mvba_two_view against the NumPy restatement of
tests/_twoview_ref.py, relative_pose against the ground truth, and bootstrap -> BundleAdjuster end to end.  Parity margins:
100 x the host-versus-host difference (eigh against SVD) of the very scene, recorded in tests/_twoview_cases.py and
re-measured by tests/test_twoview_cpu.py."""
import numpy as np
import pytest

import _init_cases as IC
import _twoview_cases as C
import _twoview_ref as T
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster
from lib.initialization import (bootstrap, covisibility, engine_intrinsics, fundamental_matrices, relative_pose,
                                restrict_observations)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["300x8", "65x70", "dense"])
def test_covisibility_counts_are_exact(name):
    pt_ptr, cam, m, n = C.count_cases()[name]
    count, tm = _mvba.covisibility(pt_ptr, cam, m, n_points=n if pt_ptr is None else None)
    want = T.covisibility(pt_ptr, cam, m, n)
    np.testing.assert_array_equal(count, want)
    assert count.dtype == np.int64 and np.array_equal(count, count.T) and tm["kernel"] > 0
    if pt_ptr is not None:
        np.testing.assert_array_equal(covisibility(pt_ptr, cam, m), want)
        np.testing.assert_array_equal(np.diag(count), np.bincount(cam, minlength=m))


def test_covisibility_beyond_the_lds_table():
    """129 cameras: m^2 x 4 bytes no longer fit the 64 KiB table, the counters are device-memory atomics."""
    rng = np.random.default_rng(3)
    vis = rng.random((200, 129)) < 0.1
    vis[:, :2] = True
    pt, cam = np.nonzero(vis)
    pt_ptr = np.concatenate([[0], np.cumsum(vis.sum(axis=1))]).astype(np.int64)
    count, _ = _mvba.covisibility(pt_ptr, cam.astype(np.int32), 129)
    np.testing.assert_array_equal(count, vis.T.astype(np.int64) @ vis.astype(np.int64))


@pytest.mark.parametrize("name", sorted(C.TWOVIEW_HOST_DIFF))
def test_fundamental_parity(name):
    pt_ptr, cam, xy, m, pairs = C.case(name)
    F, q, ns, st, tm = _mvba.two_view(pt_ptr, cam, xy, m, pairs)
    Fr, qr, nr, sr = C.reference(name)
    np.testing.assert_array_equal(ns, nr)
    np.testing.assert_array_equal(st, sr)
    bad = sr != 0
    assert np.isnan(F[bad]).all() and np.isnan(q[bad]).all() and (~bad).any()
    margin = C.MARGIN * C.TWOVIEW_HOST_DIFF[name]  # 100 x the host-versus-host difference of this scene
    d = np.abs(F[~bad] - Fr[~bad]).max()
    # the Sampson RMS under the same margin, relative to its own size; with exactly 8 points the fit is exact and the figure
    # is rounding of the order eps x |xy|, compared on that scale
    scale = np.where(nr[~bad] > 8, qr[~bad, 0], np.abs(xy).max())
    dq = (np.abs(q[~bad, 0] - qr[~bad, 0]) / scale).max()
    dr = np.abs(q[~bad, 1] - qr[~bad, 1]).max()
    print(f"{name}: max |dF| {d:.3e}, Sampson RMS relative {dq:.3e}, ratio {dr:.3e} (margin {margin:.1e})")
    assert d <= margin and dq <= margin and dr <= margin
    assert set(tm) == {"upload", "kernel", "download"} and tm["kernel"] > 0
    if name == "300x8":  # the public call, and the dense grid through pt_ptr = None
        F2, info = fundamental_matrices(pt_ptr, cam, xy, m, pairs)
        assert F2.tobytes() == F.tobytes() and set(info) == {"status", "quality", "n_shared", "timings_ms"}
    if name == "257x2":
        F3 = _mvba.two_view(None, None, xy.reshape(257, 2, 2), 2, pairs)[0]
        assert F3.tobytes() == F.tobytes()


def test_status_cases():
    pt_ptr, cam, xy, m, pairs = C.case("65x12")
    F, q, ns, st, _ = _mvba.two_view(pt_ptr, cam, xy, m, pairs)
    seven, eight = np.nonzero(ns == 7)[0], np.nonzero(ns == 8)[0]
    assert len(seven) and len(eight)
    assert (st[seven] == 1).all() and np.isnan(F[seven]).all() and np.isnan(q[seven]).all()
    assert (st[eight] == 0).all() and np.isfinite(F[eight]).all()
    for name in ("planar", "same_centre"):  # noise-free: a null space of dimension 3
        pt_ptr, cam, xy, m, pair = C.degenerate_case(name)
        F, q, ns, st, _ = _mvba.two_view(pt_ptr, cam, xy, m, [pair])
        assert st[0] == 2 and ns[0] == len(pt_ptr) - 1 and np.isnan(F).all() and np.isnan(q).all(), name


def test_bad_arguments():
    pt_ptr, cam, xy, m, _ = C.case("300x8")
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        _mvba.two_view(pt_ptr, cam, xy, m, [(0, 1), (4, 4)])
    with pytest.raises(ValueError, match=r"\(1, 8\).*n_images = 8"):
        _mvba.two_view(pt_ptr, cam, xy, m, [(1, 8)])
    with pytest.raises(ValueError, match=r"\(-1, 2\)"):
        _mvba.two_view(pt_ptr, cam, xy, m, [(-1, 2)])
    bad = cam.copy()
    bad[[0, 1]] = bad[[1, 0]]  # point 0's run no longer ascends
    with pytest.raises(ValueError, match="not ascending within point 0"):
        _mvba.two_view(pt_ptr, bad, xy, m, [(0, 1)])
    F, q, ns, st, _ = _mvba.two_view(pt_ptr, cam, xy, m, np.zeros((0, 2), np.int32))
    assert F.shape == (0, 3, 3) and st.shape == (0,)


def test_two_calls_are_bitwise_equal():
    for name in ("300x8", "5000x3"):
        pt_ptr, cam, xy, m, pairs = C.case(name)
        a, b = _mvba.two_view(pt_ptr, cam, xy, m, pairs), _mvba.two_view(pt_ptr, cam, xy, m, pairs)
        for u, v in zip(a[:4], b[:4]):
            assert u.tobytes() == v.tobytes()
        one = _mvba.two_view(pt_ptr, cam, xy, m, pairs[1:2])  # a pair's result does not depend on the other pairs of the call
        assert one[0].tobytes() == a[0][1:2].tobytes() and one[1].tobytes() == a[1][1:2].tobytes()


def test_relative_pose_recovers_the_ground_truth():
    sc = C.scene("noise_free")
    R, t, X, info = relative_pose(sc.pt_ptr, sc.cam_idx, sc.xy, sc.K_gt, (0, 1))
    Rg, tg = C.true_relative_pose(sc, 0, 1)
    e = max(np.abs(R[1] - Rg).max(), np.abs(t[1] - tg).max())
    print(f"pose error {e:.3e} (margin {C.pose_margin():.1e}), |F - E_gt| {np.abs(info['F'] - C.true_essential(sc, 0, 1)).max():.3e}")
    assert info["status"] == 0 and sorted(info["n_front"]) == [0, 0, 0, info["n_shared"]] and info["n_shared"] == 80
    assert e <= C.pose_margin()
    np.testing.assert_array_equal(R[0], np.eye(3))
    assert (t[0] == 0).all() and abs(np.linalg.norm(t[1]) - 1.0) < 1e-14
    ids = np.isfinite(X).all(axis=1)
    s = np.linalg.norm(sc.t_gt[1] - sc.t_gt[0])
    assert ids.sum() == 80 and np.isfinite(info["quality"][ids]).all() and np.isnan(info["quality"][~ids]).all()
    np.testing.assert_allclose(X[ids], ((sc.X_gt - sc.t_gt[0]) @ sc.R_gt[0])[ids] / s, rtol=0, atol=1e-11)
    # the reversed pair: camera 1 at the origin
    R2, t2, _, i2 = relative_pose(sc.pt_ptr, sc.cam_idx, sc.xy, sc.K_gt, (1, 0))
    Rg, tg = C.true_relative_pose(sc, 1, 0)
    assert i2["status"] == 0 and max(np.abs(R2[1] - Rg).max(), np.abs(t2[1] - tg).max()) <= C.pose_margin()
    # too few shared points: the two-view status comes through
    pt_ptr, cam, xy, m, pairs = C.case("65x12")
    p = pairs[np.nonzero(C.reference("65x12")[2] == 7)[0][0]]
    assert relative_pose(pt_ptr, cam, xy, np.tile(np.eye(3), (12, 1, 1)), p)[3]["status"] == 1


def _ground_truth_cost(sc, xy, K, f0):
    eng = _mvba.HipEngine(sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, xy, f0, "x-up_z-forward")
    eng.set_params(sc.X_gt, K[:, 0, 0], K[:, :2, 2], sc.t_gt, sc.R_gt)
    E = eng.cost()
    eng.close()
    return E


@pytest.mark.parametrize("units", ["unit", "pixels"])
def test_bootstrap_then_bundle_adjustment_beats_the_ground_truth(units):
    """Feature tracks and rough intrinsics in, a BA solution out: the final cost must lie below the cost of the ground truth
    on the same observations (the least-squares minimum lies about (3N + 9m - 7) / (2 n_obs) below it, a wrong basin orders
    of magnitude above)."""
    sc = C.scene("300x8")
    if units == "unit":
        xy, init_K, K_gt, f0 = sc.xy, sc.init_K, sc.K_gt, 1.0
    else:
        _, xy, init_K, _ = IC.pixel_scene()
        f0 = IC.PIXEL_F0
        K_gt = init_K.copy()
        K_gt[:, 0, 0] = K_gt[:, 1, 1] = f0 * sc.K_gt[:, 0, 0]
    K, R, t, X, info = bootstrap(sc.pt_ptr, sc.cam_idx, xy, init_K, f0=f0)
    assert info["camera_ok"].all() and info["point_ok"].all(), (info["order"], int(info["point_ok"].sum()))
    assert sorted(info["order"]) == list(range(8)) and info["order"][:2] == list(info["start_pair"])
    np.testing.assert_array_equal(K, init_K)
    np.testing.assert_allclose(R[0], np.eye(3), rtol=0, atol=1e-15)
    assert np.abs(t[0]).max() < 1e-15 and abs(np.linalg.norm(t[1]) - 1.0) < 1e-14
    g = 0 if info["axis"] == "x-right_z-forward" else 1
    assert abs(t[1, g]) == np.abs(t[1, :2]).max()
    ba = BundleAdjuster.from_observations(300, 8, sc.pt_ptr, sc.cam_idx, xy, X, K, R, t, f0=f0, axis=info["axis"])
    E0 = ba._engine.cost()
    ba.optimize()
    E, E_gt = ba._engine.cost(), _ground_truth_cost(sc, xy, K_gt, f0)
    print(f"{units}: start pair {info['start_pair']}, order {info['order']}, axis {info['axis']}: cost {E0:.4e} -> {E:.4e}, ground truth {E_gt:.4e}")
    assert E < E_gt


def test_partial_bootstrap():
    """Camera 5 sees 9 points (< min_points = 12): it comes back camera_ok = False and NaN, and the rest is what the run
    without it gives after restrict_observations.  The same with camera 1 raises."""
    sc = C.scene("300x8")
    pt_ptr, cam, xy = C.short_camera_scene(5)
    K, R, t, X, info = bootstrap(pt_ptr, cam, xy, sc.init_K)
    rest = np.arange(8) != 5
    assert info["camera_ok"].tolist() == rest.tolist() and 5 not in info["order"]
    assert np.isnan(R[5]).all() and np.isnan(t[5]).all() and np.isfinite(R[rest]).all()
    p2, c2, xy2, pid, cid = restrict_observations(pt_ptr, cam, xy, np.ones(300, bool), rest)
    assert cid.tolist() == [0, 1, 2, 3, 4, 6, 7] and len(pid) == 300
    K2, R2, t2, X2, i2 = bootstrap(p2, c2, xy2, sc.init_K[rest])
    assert i2["camera_ok"].all() and [int(cid[c]) for c in i2["order"]] == info["order"]
    np.testing.assert_array_equal(i2["point_ok"], info["point_ok"])
    ok = info["point_ok"]
    for got, want in ((R[rest], R2), (t[rest], t2), (X[ok], X2[ok])):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)  # (the same device calls on the same numbers)
    assert np.isnan(X[~ok]).all()
    with pytest.raises(ValueError, match="camera 1"):
        bootstrap(*C.short_camera_scene(1), sc.init_K)
    with pytest.raises(ValueError, match="no start pair"):
        bootstrap(pt_ptr, cam, xy, sc.init_K, start_pair=(0, 5))
