"""Calibrated robust resection on the device: mvba_pose_robust and mvba_pose_refine against the NumPy
restatement of tests/_pose_ransac_ref.py -- count tables (but for the hypotheses on which the two host root finders disagree:
at most 1 % of a table, never a best one), best hypotheses, usable and inlier counts, statuses and the inlier bytes EXACTLY
(tests/test_pose_ransac_cpu.py asserts the premises under which that may be asked), R, t and the RMS within 100 x the
host-versus-host difference of the very case (tests/_pose_ransac_cases.py) --, its structure (camera lists, tiles, refit
counts, bad arguments), and bootstrap with ``pose_threshold`` on contaminated tracks."""
import numpy as np
import pytest

import _init_cases as IC
import _pose_ransac_cases as PC
import _resect_ransac_cases as QC
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster
from lib.initialization import bootstrap, refine_poses, restrict_observations, robust_pose_cameras

pytestmark = pytest.mark.gpu

KEYS = ("R", "t", "quality", "n_usable", "n_inliers", "best", "status", "inlier", "hyp_count")


def _run(X, pt_ptr, cam, xy, K, thr, H, seed, n_refit=2, **kw):
    return _mvba.pose_robust(X, pt_ptr, cam, xy, K, thr, n_hypotheses=H, seed=seed, n_refit=n_refit, return_counts=True, **kw)


def _assert_exact(got, want, other, what):
    firm = ~PC.fragile(want, other)
    np.testing.assert_array_equal(got["hyp_count"][firm], want["hyp_count"][firm], err_msg=f"{what}: hyp_count")
    for key in ("best", "n_usable", "n_inliers", "status", "inlier"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")


def _assert_close(got, want, margin, what):
    ok = want["status"] == 0
    bad = ~ok
    assert np.isnan(got["R"][bad]).all() and np.isnan(got["t"][bad]).all() and np.isnan(got["quality"][bad]).all()
    assert (got["n_inliers"][bad] == 0).all()
    if not ok.any():
        return
    d = max(np.abs(got["R"][ok] - want["R"][ok]).max(), np.abs(got["t"][ok] - want["t"][ok]).max())
    dq = np.abs(got["quality"][ok, 0] - want["quality"][ok, 0]).max()
    print(f"{what}: max |d(R, t)| {d:.3e}, RMS {dq:.3e} (margin {margin:.1e})")
    assert d <= margin and dq <= margin


@pytest.mark.parametrize("name", sorted(PC.PARITY))
def test_parity(name):
    X, pt_ptr, cam, xy, K, thr, H, seed, hit = PC.case(name)
    got, want, other = _run(X, pt_ptr, cam, xy, K, thr, H, seed), PC.reference(name), PC.other(PC.reference, name)
    _assert_exact(got, want, other, name)
    _assert_close(got, want, PC.MARGIN * PC.POSE_HOST_DIFF[name], name)
    assert set(got["timings_ms"]) == {"upload", "score", "refit", "other"} and got["timings_ms"]["score"] > 0
    if name == "coplanar_noisy":  # exactly the clean sets, on data where the DLT has status 2
        assert (got["status"] == 0).all()
        np.testing.assert_array_equal(got["inlier"], ~hit)
        assert (_mvba.resect_robust(X, pt_ptr, cam, xy, 3, thr, n_hypotheses=H, seed=seed)["status"] == 2).all()
    if name in ("300x8", "pixels"):  # the public call
        R, t, info = robust_pose_cameras(X, pt_ptr, cam, xy, K, thr, n_hypotheses=H, seed=seed)
        assert R.tobytes() == got["R"].tobytes() and t.tobytes() == got["t"].tobytes() and np.array_equal(info["inlier"], got["inlier"])
        w = want["n_inliers"] / want["n_usable"]
        np.testing.assert_allclose(info["confidence"], 1.0 - (1.0 - w ** 4) ** H, rtol=1e-12)
    if name == "300x8":  # without refits: the best hypothesis's own pose
        got0, want0 = _run(X, pt_ptr, cam, xy, K, thr, H, seed, n_refit=0), PC.reference(name, n_refit=0)
        _assert_exact(got0, want0, PC.other(PC.reference, name, n_refit=0), name + ", n_refit = 0")
        np.testing.assert_array_equal(got0["n_inliers"], got0["hyp_count"].max(axis=1))
        _assert_close(got0, want0, PC.MARGIN * PC.POSE_HOST_DIFF["300x8_refit0"], name + ", n_refit = 0")
        assert (got0["quality"][:, 1] == 0).all()
        for key in ("hyp_count", "best"):  # (hypotheses and scores do not depend on the refits)
            assert got0[key].tobytes() == got[key].tobytes()
        again = _run(X, pt_ptr, cam, xy, K, thr, H, seed)  # two calls are bitwise equal
        for key in KEYS:
            assert again[key].tobytes() == got[key].tobytes(), key
        moved = _run(X, pt_ptr, cam, xy, K, thr, H, seed + 1)
        assert not np.array_equal(got["hyp_count"], moved["hyp_count"])
    if name == "dense":  # the dense grid and the list form are one computation
        p, c = IC.ref.dense_list(len(X), len(K))
        listed = _run(X, p, c, np.asarray(xy).reshape(-1, 2), K, thr, H, seed)
        for key in KEYS:
            assert listed[key].tobytes() == got[key].tobytes(), key


def test_camera_tiles_under_the_byte_bound():
    """One camera of "300x8" listed 11 times at 65536 hypotheses: 128 MiB / (196 x 65536) = 10 cameras per tile, so the call takes
    two; every occurrence is bitwise the first (QC.camera_tile's docstring says what the restated formula can and cannot show).
    The first 512 counts are those of the parity case: a hypothesis depends on (seed, camera, h) alone."""
    X, pt_ptr, cam, xy, K, thr, _, seed, _ = PC.case("300x8")
    H, k = 65536, 5
    assert PC.camera_tile(11, H) == 10
    got = _run(X, pt_ptr, cam, xy, K, thr, H, seed, cameras=[k] * 11)
    assert (got["status"] == 0).all()
    for key in KEYS:
        if key != "inlier":
            for i in range(1, 11):
                assert got[key][i].tobytes() == got[key][0].tobytes(), (key, i)
    assert got["inlier"].sum() == got["n_inliers"][0] and (cam[got["inlier"]] == k).all()
    want, other = PC.reference("300x8"), PC.other(PC.reference, "300x8")
    firm = ~PC.fragile(want, other)[k]
    np.testing.assert_array_equal(got["hyp_count"][0][:512][firm], want["hyp_count"][k][firm])
    assert got["best"][0] == np.argmax(got["hyp_count"][0])


@pytest.mark.parametrize("name", PC.STATUS_NAMES)
def test_status_shapes(name):
    X, pt_ptr, cam, xy, K, ok, _ = PC.status_case(name)
    got = _run(X, pt_ptr, cam, xy, K, PC.THRESHOLD, PC.STATUS_HYP, PC.STATUS_SEED, point_ok=ok)
    want = PC.status_reference(name)
    _assert_exact(got, want, PC.other(PC.status_reference, name), name)
    if name == "collinear":
        assert (got["status"] == 2).all() and np.isnan(got["R"]).all() and not got["inlier"].any() and (got["hyp_count"] == -1).all()
    else:
        _assert_close(got, want, PC.MARGIN * PC.POSE_HOST_DIFF[name], name)
    bad = got["status"] != 0
    assert (got["n_inliers"][bad] == 0).all() and not got["inlier"][np.isin(cam, np.nonzero(bad)[0])].any()
    if name == "four":
        assert got["status"].tolist() == [0, 0, 1, 0] and (got["hyp_count"][1] == 4).all() and (got["hyp_count"][2] == -1).all()
    if name == "empty":
        assert (got["status"][list(IC.EMPTY_CAMERAS)] == 1).all()


def test_camera_list_with_duplicates():
    X, pt_ptr, cam, xy, K, thr, H, seed, _ = PC.case("300x8")
    got = _run(X, pt_ptr, cam, xy, K, thr, H, seed, cameras=[5, 2, 5])
    full = _run(X, pt_ptr, cam, xy, K, thr, H, seed)
    for i, k in enumerate((5, 2, 5)):  # a camera's result does not depend on which other cameras are listed
        for key in KEYS:
            if key != "inlier":
                assert full[key][k].tobytes() == got[key][i].tobytes(), (k, key)
    np.testing.assert_array_equal(got["inlier"], full["inlier"] & np.isin(cam, (2, 5)))
    none = _run(X, pt_ptr, cam, xy, K, thr, H, seed, cameras=[])
    assert none["R"].shape == (0, 3, 3) and not none["inlier"].any()


@pytest.mark.parametrize("n_refit", PC.REFIT_COUNTS)
def test_refit_counts(n_refit):
    X, pt_ptr, cam, xy, K, _, H, seed, _ = PC.case("5000x3")
    got, want = _run(X, pt_ptr, cam, xy, K, PC.REFIT_THRESHOLD, H, seed, n_refit=n_refit), PC.refit_reference(n_refit)
    _assert_exact(got, want, PC.other(PC.refit_reference, n_refit), f"n_refit = {n_refit}")
    _assert_close(got, want, PC.MARGIN * PC.REFIT_TRACE_DIFF[n_refit], f"n_refit = {n_refit}")


def test_refine_poses():
    X, pt_ptr, cam, xy, K, R0, t0 = PC.refine_case()
    Rw, tw, qw, nw, sw = PC.refine_reference()
    R, t, info = refine_poses(X, pt_ptr, cam, xy, K, R0, t0, n_steps=PC.REFINE_STEPS)
    d = max(np.abs(R - Rw).max(), np.abs(t - tw).max())
    print(f"refine: max |d(R, t)| {d:.3e} (margin {PC.MARGIN * PC.REFINE_HOST_DIFF:.1e}), RMS {info['quality'][:, 0].max():.2e} -> "
          f"{info['quality'][:, 1].max():.2e}, steps {info['quality'][:, 2].tolist()}")
    assert (info["status"] == 0).all() and d <= PC.MARGIN * PC.REFINE_HOST_DIFF
    assert (info["quality"][:, 1] <= info["quality"][:, 0]).all()
    np.testing.assert_allclose(info["quality"][:, :2], qw[:, :2], rtol=0, atol=PC.MARGIN * PC.REFINE_HOST_DIFF)
    np.testing.assert_array_equal(info["n_usable"], nw)
    again = refine_poses(X, pt_ptr, cam, xy, K, R0, t0, n_steps=PC.REFINE_STEPS)
    assert again[0].tobytes() == R.tobytes() and again[1].tobytes() == t.tobytes()
    # obs_ok = the inlier mask of robust_pose_cameras, n_steps = 0: the poses come back bitwise
    Xc, pc, cc, xyc, Kc, thr, H, seed, _ = PC.case("300x8")
    Rr, tr, ri = robust_pose_cameras(Xc, pc, cc, xyc, Kc, thr, n_hypotheses=H, seed=seed)
    R1, t1, i1 = refine_poses(Xc, pc, cc, xyc, Kc, Rr, tr, obs_ok=ri["inlier"], n_steps=0)
    assert R1.tobytes() == Rr.tobytes() and t1.tobytes() == tr.tobytes() and (i1["status"] == 0).all() and (i1["quality"][:, 2] == 0).all()
    np.testing.assert_array_equal(i1["n_usable"], ri["n_inliers"])
    np.testing.assert_allclose(i1["quality"][:, 0], ri["quality"][:, 0], rtol=1e-12)
    # statuses 1 and 2: two observations left to camera 2, a NaN in camera 5's pose; both keep their input
    few = cam != 2
    few[np.nonzero(cam == 2)[0][:2]] = True
    tn = t0.copy()
    tn[5, 1] = np.nan
    R2, t2, i2 = refine_poses(X, pt_ptr, cam, xy, K, R0, tn, obs_ok=few)
    assert i2["status"].tolist() == [0, 0, 1, 0, 0, 2, 0, 0] and i2["n_usable"][2] == 2 and np.isnan(i2["quality"][[2, 5]]).all()
    assert R2[[2, 5]].tobytes() == R0[[2, 5]].tobytes() and t2[2].tobytes() == t0[2].tobytes() and np.isnan(t2[5, 1])
    # a listed subset, with a duplicate
    R3, t3, i3 = refine_poses(X, pt_ptr, cam, xy, K, R0[[6, 1, 6]], t0[[6, 1, 6]], cameras=[6, 1, 6], n_steps=PC.REFINE_STEPS)
    assert R3.tobytes() == R[[6, 1, 6]].tobytes() and t3.tobytes() == t[[6, 1, 6]].tobytes()


def test_bad_arguments():
    X, pt_ptr, cam, xy, K, thr, _, _, _ = PC.case("300x8")
    for kw, text in (({"threshold": 0.0}, "threshold = 0.0"), ({"threshold": np.inf}, "threshold = inf"), ({"n_hypotheses": 0}, "n_hypotheses = 0"),
                     ({"n_hypotheses": 65537}, "n_hypotheses = 65537"), ({"n_refit": -1}, "n_refit = -1"), ({"n_refit": 17}, "n_refit = 17"),
                     ({"n_refine": -1}, "n_refine = -1"), ({"n_refine": 17}, "n_refine = 17"), ({"cameras": [0, 8]}, "cameras\\[1\\] = 8")):
        args = {"threshold": thr, "n_hypotheses": 16, "n_refit": 2}
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            _mvba.pose_robust(X, pt_ptr, cam, xy, K, args.pop("threshold"), **args)
    with pytest.raises(ValueError, match="n_steps = 65"):
        _mvba.pose_refine(X, pt_ptr, cam, xy, K, np.tile(np.eye(3), (8, 1, 1)), np.zeros((8, 3)), n_steps=65)
    import ctypes as C

    lib = _mvba.load_library()
    Xc, xyc = np.ascontiguousarray(X), np.ascontiguousarray(xy)
    R, t = np.empty((8, 9)), np.empty((8, 3))
    rc = lib.mvba_pose_robust(_mvba._ptr(Xc), 300, pt_ptr.ctypes.data_as(C.POINTER(C.c_int64)), cam.ctypes.data_as(C.POINTER(C.c_int32)),
                              _mvba._ptr(xyc), len(cam), 8, None, None, None, 8, thr, 16, 1, 5, 2, _mvba._ptr(R), _mvba._ptr(t), None, None, None,
                              None, None, None, None, None, -1)
    assert rc == _mvba.MVBA_ERR_BADARG and "null argument: K (argument 9)" in lib.mvba_last_error().decode()


def _robust_cost(n, pt_ptr, cam, xy, X, K, R, t, delta):
    eng = _mvba.HipEngine(n, 8, pt_ptr, cam, xy, 1.0, "x-up_z-forward", loss="huber", loss_scale=delta)
    eng.set_params(X, K[:, 0, 0], K[:, :2, 2], t, R)
    E = eng.cost()
    eng.close()
    return E


def test_bootstrap_with_calibrated_registration_then_robust_bundle_adjustment():
    """20 % of the observations of cameras 2 .. 7 replaced: with ``pose_threshold`` all 8 cameras are registered, in the
    reference's order, from clean observations only, and Huber BA from there ends below the cost of the ground truth."""
    sc, xy, replaced = QC.bootstrap_case()
    with pytest.raises(ValueError, match="pose_threshold and resect_threshold"):
        bootstrap(sc.pt_ptr, sc.cam_idx, xy, sc.init_K, start_pair=(0, 1), pose_threshold=0.01, resect_threshold=0.01)
    K, R, t, X, info = bootstrap(sc.pt_ptr, sc.cam_idx, xy, sc.init_K, start_pair=(0, 1), max_rms=0.01, pose_threshold=PC.THRESHOLD, seed=1)
    Rr, tr, Xr, ir = PC.reference_bootstrap()
    assert info["order"] == ir["order"] and info["camera_ok"].all() and len(info["order"]) == 8
    for key in ("camera_ok", "point_ok", "obs_ok", "inlier"):
        np.testing.assert_array_equal(info[key], ir[key], err_msg=key)
    assert not (info["inlier"] & replaced).any()
    ok = info["point_ok"]
    d = max(np.abs(R - Rr).max(), np.abs(t - tr).max())
    e = QC.pose_error(sc, R, t, info["camera_ok"])
    print(f"bootstrap: {ok.sum()} points, |d| to the reference {d:.2e} (margin {PC.MARGIN * PC.BOOT_HOST_DIFF:.1e}), pose error R {e[0]:.3e} "
          f"t {e[1]:.3e}")
    assert d <= PC.MARGIN * PC.BOOT_HOST_DIFF and np.abs(X[ok] - Xr[ok]).max() <= PC.MARGIN * PC.BOOT_HOST_DIFF
    assert max(e) <= QC.BOOT_FACTOR * QC.BOOT_CLEAN_ERR
    assert K.tobytes() == np.asarray(sc.init_K, np.float64).tobytes()
    ptr, cam, z, pid, _ = restrict_observations(sc.pt_ptr, sc.cam_idx, xy, ok, info["camera_ok"])
    delta = 5e-3  # five times the noise: the replaced observations are far beyond it
    ba = BundleAdjuster.from_observations(len(pid), 8, ptr, cam, z, X[pid], K, R, t, axis=info["axis"], loss="huber", loss_scale=delta)
    E0 = ba._engine.cost()
    ba.optimize()
    E, E_gt = ba._engine.cost(), _robust_cost(len(pid), ptr, cam, z, sc.X_gt[pid], sc.K_gt, sc.R_gt, sc.t_gt, delta)
    print(f"huber cost {E0:.4e} -> {E:.4e}, ground truth {E_gt:.4e}")
    assert E < E_gt
