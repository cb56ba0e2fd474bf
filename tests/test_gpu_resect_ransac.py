"""Robust resection on the device: mvba_resect_robust against the NumPy restatement of
tests/_resect_ransac_ref.py -- count tables, best hypotheses, usable and inlier counts, statuses and the inlier bytes EXACTLY
(tests/test_resect_ransac_cpu.py asserts the premises under which that may be asked), P and quality within 100 x the
host-versus-host difference of the very case (tests/_resect_ransac_cases.py) --, its structure (camera lists, tiles, seeds,
refit counts, the largest hypothesis count, bad arguments), and bootstrap with ``resect_threshold`` on contaminated tracks.

The RMS residual is compared absolutely, within the margin of P: a change dP of a matrix with |P[2, :3]| = 1 moves a
reprojection of a point at depth and distance of order 1 by about |dP| in the units of xy, and the RMS by no more (the "six"
shape is noise-free: its RMS is rounding, and a relative figure would say nothing)."""
import numpy as np
import pytest

import _init_cases as IC
import _resect_ransac_cases as QC
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster
from lib.initialization import bootstrap, decompose_projection, restrict_observations, robust_resect_cameras

pytestmark = pytest.mark.gpu

KEYS = ("P", "quality", "n_usable", "n_inliers", "best", "status", "inlier", "hyp_count")


def _run(X, pt_ptr, cam, xy, m, thr, H, seed, n_refit=2, **kw):
    return _mvba.resect_robust(X, pt_ptr, cam, xy, m, thr, n_hypotheses=H, seed=seed, n_refit=n_refit, return_counts=True, **kw)


def _assert_exact(got, want, what):
    for key in ("hyp_count", "best", "n_usable", "n_inliers", "status", "inlier"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")


def _assert_close(got, want, margin, what):
    ok = want["status"] == 0
    bad = ~ok
    assert np.isnan(got["P"][bad]).all() and np.isnan(got["quality"][bad]).all()
    if not ok.any():
        return
    d = np.abs(got["P"][ok] - want["P"][ok]).max()
    dq = np.abs(got["quality"][ok] - want["quality"][ok]).max(axis=0)
    print(f"{what}: max |dP| {d:.3e}, RMS {dq[0]:.3e}, ratio {dq[1]:.3e} (margin {margin:.1e})")
    assert d <= margin and dq[0] <= margin and dq[1] <= margin


@pytest.mark.parametrize("name", sorted(QC.PARITY))
def test_parity(name):
    X, pt_ptr, cam, xy, m, thr, H, seed, f0, _ = QC.case(name)
    got, want = _run(X, pt_ptr, cam, xy, m, thr, H, seed), QC.reference(name)
    _assert_exact(got, want, name)
    _assert_close(got, want, QC.MARGIN * QC.RESECT_RANSAC_HOST_DIFF[name], name)
    assert set(got["timings_ms"]) == {"upload", "score", "refit", "other"} and got["timings_ms"]["score"] > 0
    if name in ("300x8", "pixels"):  # the public call
        K, R, t, info = robust_resect_cameras(X, pt_ptr, cam, xy, m, thr, f0=f0, n_hypotheses=H, seed=seed)
        assert info["P"].tobytes() == got["P"].tobytes() and np.array_equal(info["inlier"], got["inlier"])
        w = want["n_inliers"] / want["n_usable"]
        np.testing.assert_allclose(info["confidence"], 1.0 - (1.0 - w ** 6) ** H, rtol=1e-12)
        Kd, Rd, td = decompose_projection(got["P"], f0)
        assert K.tobytes() == Kd.tobytes() and R.tobytes() == Rd.tobytes() and t.tobytes() == td.tobytes() and (K[:, 2, 2] == f0).all()
    if name == "300x8":  # without refits: the best hypothesis itself
        got0, want0 = _run(X, pt_ptr, cam, xy, m, thr, H, seed, n_refit=0), QC.reference(name, "eigh", 0)
        _assert_exact(got0, want0, name + ", n_refit = 0")
        np.testing.assert_array_equal(got0["n_inliers"], got0["hyp_count"].max(axis=1))
        _assert_close(got0, want0, QC.MARGIN * QC.RESECT_RANSAC_HOST_DIFF["300x8_refit0"], name + ", n_refit = 0")
        assert (got0["quality"][:, 1] == 0).all()
    if name == "dense":  # the dense grid and the list form are one computation
        p, c = IC.ref.dense_list(len(X), m)
        listed = _run(X, p, c, np.asarray(xy).reshape(-1, 2), m, thr, H, seed)
        for key in KEYS:
            assert listed[key].tobytes() == got[key].tobytes(), key


def test_camera_tiles_under_the_byte_bound():
    """"900x300" at 8192 hypotheses: 128 MiB / (100 x 8192) = 163 cameras per tile, so the call takes two; the cameras at the
    ends of both tiles are bitwise what a call listing each alone returns.  The 163 is the formula restated in Python
    (QC.camera_tile): the library does not report its tile size and results do not depend on it, so what this test shows is
    that a call which the formula makes split returns, for every camera compared, what the unsplit single-camera call returns
    -- a wrong offset between tiles would fail it; a tile size other than the documented one would not."""
    X, pt_ptr, cam, xy, m, thr, _, seed, _, _ = QC.case("900x300")
    H = 8192
    assert QC.camera_tile(m, H) == 163 < m <= 2 * 163
    full = _run(X, pt_ptr, cam, xy, m, thr, H, seed)
    assert (full["status"] == 0).all()
    union = np.zeros(len(cam), bool)
    for k in (0, 162, 163, 299):
        one = _run(X, pt_ptr, cam, xy, m, thr, H, seed, cameras=[k])
        for key in KEYS:
            if key != "inlier":
                assert one[key][0].tobytes() == full[key][k].tobytes(), (k, key)
        np.testing.assert_array_equal(one["inlier"], full["inlier"] & (cam == k))
        union |= one["inlier"]
    assert union.sum() == full["n_inliers"][[0, 162, 163, 299]].sum()


@pytest.mark.parametrize("name", QC.STATUS_NAMES)
def test_status_shapes(name):
    X, pt_ptr, cam, xy, m, ok, _ = QC.status_case(name)
    got = _run(X, pt_ptr, cam, xy, m, QC.THRESHOLD, QC.STATUS_HYP, QC.STATUS_SEED, point_ok=ok)
    want = QC.status_reference(name)
    _assert_exact(got, want, name)
    if name == "coplanar":
        assert (got["status"] == 2).all() and np.isnan(got["P"]).all() and not got["inlier"].any() and (got["hyp_count"] == -1).all()
    else:
        _assert_close(got, want, QC.MARGIN * QC.RESECT_RANSAC_HOST_DIFF[name], name)
    bad = got["status"] != 0
    assert (got["n_inliers"][bad] == 0).all() and not got["inlier"][np.isin(cam, np.nonzero(bad)[0])].any()
    if name == "six":
        assert got["status"].tolist() == [0, 0, 1, 0] and (got["hyp_count"][1] == 6).all() and (got["hyp_count"][2] == -1).all()
    if name == "all_replaced":
        assert got["status"][QC.ALL_REPLACED_CAMERA] == 4


def test_camera_list_with_duplicates():
    X, pt_ptr, cam, xy, m, thr, H, seed, _, _ = QC.case("300x8")
    got = _run(X, pt_ptr, cam, xy, m, thr, H, seed, cameras=[5, 2, 5])
    full = QC.reference("300x8")
    for i, k in enumerate((5, 2, 5)):
        one = _run(X, pt_ptr, cam, xy, m, thr, H, seed, cameras=[k])
        for key in KEYS:
            if key != "inlier":
                assert one[key][0].tobytes() == got[key][i].tobytes(), (k, key)
        np.testing.assert_array_equal(one["inlier"], got["inlier"] & (cam == k))
        np.testing.assert_array_equal(got["hyp_count"][i], full["hyp_count"][k])
    np.testing.assert_array_equal(got["inlier"], full["inlier"] & np.isin(cam, (2, 5)))
    none = _run(X, pt_ptr, cam, xy, m, thr, H, seed, cameras=[])
    assert none["P"].shape == (0, 3, 4) and not none["inlier"].any()


def test_two_calls_are_bitwise_equal_and_the_seed_moves_the_sample():
    for name in ("300x8", "5000x3"):
        X, pt_ptr, cam, xy, m, thr, H, seed, _, _ = QC.case(name)
        a, b = _run(X, pt_ptr, cam, xy, m, thr, H, seed), _run(X, pt_ptr, cam, xy, m, thr, H, seed)
        for key in KEYS:
            assert a[key].tobytes() == b[key].tobytes(), (name, key)
        c = _run(X, pt_ptr, cam, xy, m, thr, H, seed + 1)
        assert not np.array_equal(a["hyp_count"], c["hyp_count"]) and not np.array_equal(a["best"], c["best"])


def test_max_hypotheses():
    """n_hypotheses = 65536 on one camera of "300x8": 1024 workgroups of k_resect_hyp, 1024 hypothesis blocks of k_resect_score."""
    X, pt_ptr, cam, xy, m, thr, _, seed, _, _ = QC.case("300x8")
    got = _run(X, pt_ptr, cam, xy, m, thr, QC.MAX_HYP, seed, cameras=[QC.MAX_HYP_CAMERA])
    hs, counts, _, _ = QC.max_hyp_reference()
    np.testing.assert_array_equal(got["hyp_count"][0][hs], counts)
    assert got["status"][0] == 0 and got["hyp_count"][0].max() == got["hyp_count"][0][got["best"][0]]
    assert got["best"][0] == np.argmax(got["hyp_count"][0])
    np.testing.assert_array_equal(got["hyp_count"][0][:512], QC.reference("300x8")["hyp_count"][QC.MAX_HYP_CAMERA])


@pytest.mark.parametrize("n_refit", QC.REFIT_COUNTS)
def test_refit_counts(n_refit):
    X, pt_ptr, cam, xy, m, _, H, seed, _, _ = QC.case("5000x3")
    got, want = _run(X, pt_ptr, cam, xy, m, QC.REFIT_THRESHOLD, H, seed, n_refit=n_refit), QC.refit_reference(n_refit)
    _assert_exact(got, want, f"n_refit = {n_refit}")
    _assert_close(got, want, QC.MARGIN * QC.REFIT_HOST_DIFF[n_refit], f"n_refit = {n_refit}")


def test_bad_arguments():
    X, pt_ptr, cam, xy, m, thr, _, _, _, _ = QC.case("300x8")
    for kw, text in (({"threshold": 0.0}, "threshold = 0.0"), ({"threshold": np.inf}, "threshold = inf"), ({"n_hypotheses": 0}, "n_hypotheses = 0"),
                     ({"n_hypotheses": 65537}, "n_hypotheses = 65537"), ({"n_refit": -1}, "n_refit = -1"), ({"n_refit": 17}, "n_refit = 17"),
                     ({"cameras": [0, 8]}, "cameras\\[1\\] = 8"), ({"cameras": [-1]}, "cameras\\[0\\] = -1")):
        args = {"threshold": thr, "n_hypotheses": 16, "n_refit": 2}
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            _mvba.resect_robust(X, pt_ptr, cam, xy, m, args.pop("threshold"), **args)
    bad_cam = cam.copy()
    bad_cam[7] = m
    with pytest.raises(ValueError, match="cam_idx out of range"):
        _mvba.resect_robust(X, pt_ptr, bad_cam, xy, m, thr)


def _robust_cost(n, pt_ptr, cam, xy, X, K, R, t, delta):
    eng = _mvba.HipEngine(n, 8, pt_ptr, cam, xy, 1.0, "x-up_z-forward", loss="huber", loss_scale=delta)
    eng.set_params(X, K[:, 0, 0], K[:, :2, 2], t, R)
    E = eng.cost()
    eng.close()
    return E


def test_bootstrap_with_robust_resection_then_robust_bundle_adjustment():
    """20 % of the observations of cameras 2 .. 7 replaced: with ``resect_threshold`` all 8 cameras are registered, in the
    reference's order, from clean observations only; without it fewer are, or wrongly -- what the feature buys."""
    sc, xy, replaced = QC.bootstrap_case()
    K, R, t, X, info = bootstrap(sc.pt_ptr, sc.cam_idx, xy, sc.init_K, start_pair=(0, 1), max_rms=0.01, resect_threshold=QC.THRESHOLD, seed=1)
    Rr, tr, Xr, ir = QC.reference_bootstrap()
    assert info["order"] == ir["order"] and info["camera_ok"].all() and len(info["order"]) == 8
    for key in ("camera_ok", "point_ok", "obs_ok", "inlier"):
        np.testing.assert_array_equal(info[key], ir[key], err_msg=key)
    assert not (info["inlier"] & replaced).any()
    ok = info["point_ok"]
    d = max(np.abs(R - Rr).max(), np.abs(t - tr).max(), np.abs(X[ok] - Xr[ok]).max())
    e = max(QC.pose_error(sc, R, t, info["camera_ok"]))
    print(f"bootstrap: {ok.sum()} points, |d| to the reference {d:.2e} (margin {QC.MARGIN * QC.BOOT_HOST_DIFF:.1e}), pose error {e:.2e} "
          f"(bound {QC.BOOT_FACTOR} x {QC.BOOT_CLEAN_ERR:.1e})")
    assert d <= QC.MARGIN * QC.BOOT_HOST_DIFF
    assert e <= QC.BOOT_FACTOR * QC.BOOT_CLEAN_ERR
    ptr, cam, z, pid, _ = restrict_observations(sc.pt_ptr, sc.cam_idx, xy, ok, info["camera_ok"])
    delta = 5e-3  # five times the noise: the replaced observations are far beyond it
    ba = BundleAdjuster.from_observations(len(pid), 8, ptr, cam, z, X[pid], K, R, t, axis=info["axis"], loss="huber", loss_scale=delta)
    E0 = ba._engine.cost()
    ba.optimize()
    E, E_gt = ba._engine.cost(), _robust_cost(len(pid), ptr, cam, z, sc.X_gt[pid], sc.K_gt, sc.R_gt, sc.t_gt, delta)
    print(f"huber cost {E0:.4e} -> {E:.4e}, ground truth {E_gt:.4e}")
    assert E < E_gt
    # the same call without resect_threshold (the reference registers 4 cameras, 0 and 1 among them: it does not raise)
    _, Rp, tp, _, ip = bootstrap(sc.pt_ptr, sc.cam_idx, xy, sc.init_K, start_pair=(0, 1), max_rms=0.01, seed=1)
    assert "obs_ok" not in ip and "inlier" not in ip
    assert ip["camera_ok"].sum() < 8 or max(QC.pose_error(sc, Rp, tp, ip["camera_ok"])) > 1.0
