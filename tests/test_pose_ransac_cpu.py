"""Calibrated robust resection, the part that needs no GPU: the sample generator libmvba.so exports is the
reference's and the first 4 draws of the two-view one, the argument checks, the premises under which the GPU parity tests may
ask for EXACT count tables (margins, fragile hypotheses), what the reference recovers, and the host-versus-host figures that
tests/_pose_ransac_cases.py records."""
import ctypes
import os

import numpy as np
import pytest

import _init_cases as IC
import _pose_ransac_cases as PC
import _pose_ransac_ref as PR
import _resect_ransac_cases as QC
import _resect_ransac_ref as QR
from lib import _mvba
from lib.initialization import pose_sample, ransac_sample

SAMPLE_TABLE = [(0, 0, 0, 4), (0, 0, 0, 5), (0, 0, 0, 7), (1, 0, 5, 80), (1, 3, 511, 157), ((1 << 64) - 1, 3, 7, (1 << 31) - 1), (7, 5, 511, 300),
                (1, 1703, 65535, 9), (12345678901234567890, 6, 3, 8)]


@pytest.mark.parametrize("seed,k,h,n", SAMPLE_TABLE)
def test_exported_sample_generator_is_the_reference(seed, k, h, n):
    """n = 4 (a permutation), n below the two-view generator's range, n = 2^31 - 1, seed = 2^64 - 1."""
    got, want = pose_sample(seed, k, h, n), PR.sample(seed, k, h, n)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int64 and len(set(got.tolist())) == 4 and (got >= 0).all() and (got < n).all()
    if n == 4:
        assert sorted(got.tolist()) == list(range(4))
    if n >= 8:  # the 8-draw instance is unchanged, and the 4 draws are its first 4
        np.testing.assert_array_equal(got, ransac_sample(seed, k, k, h, n)[:4])


def test_sample_depends_on_camera_and_seed_and_rejects_bad_arguments():
    assert not np.array_equal(pose_sample(1, 0, 5, 80), pose_sample(1, 1, 5, 80))
    assert not np.array_equal(pose_sample(1, 0, 5, 80), pose_sample(2, 0, 5, 80))
    for args, text in (((0, 0, 0, 3), "n = 3"), ((0, 0, 0, 1 << 31), "n = 2147483648"), ((0, 0, -1, 80), "h = -1"), ((0, -2, 0, 80), "k = -2")):
        with pytest.raises(ValueError, match=text):
            pose_sample(*args)


def test_library_exports_the_entry_points_and_checks_arguments_without_a_device():
    names = ("mvba_pose_robust", "mvba_pose_refine", "mvba_pose_sample")
    lib = ctypes.CDLL(_mvba.LIB_PATH)
    for name in names:
        assert name in _mvba.SIGNATURES and hasattr(lib, name), name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mvba.h")).read()
    for name in names:
        assert f"int {name}(" in hdr
    lib = _mvba.load_library()
    i32, i64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    X, pt_ptr, cam, xy, K, _, _, _, _ = PC.case("300x8")
    X, xy, K = np.ascontiguousarray(X), np.ascontiguousarray(xy), np.ascontiguousarray(K)
    R, t = np.empty((8, 9)), np.empty((8, 3))

    def robust(thr=0.01, H=16, n_refine=5, n_refit=2, cameras=None, nc=None, K=K):
        cams = None if cameras is None else np.asarray(cameras, np.int32)
        rc = lib.mvba_pose_robust(_mvba._ptr(X), 300, pt_ptr.ctypes.data_as(i64), cam.ctypes.data_as(i32), _mvba._ptr(xy), len(cam), 8, None,
                                  None if K is None else _mvba._ptr(K), None if cams is None else cams.ctypes.data_as(i32),
                                  (8 if cams is None else len(cams)) if nc is None else nc, thr, H, 1, n_refine, n_refit, _mvba._ptr(R),
                                  _mvba._ptr(t), None, None, None, None, None, None, None, None, -1)
        return rc, lib.mvba_last_error().decode()

    def refine(n_steps=10, K=K, cameras=None):
        cams = None if cameras is None else np.asarray(cameras, np.int32)
        rc = lib.mvba_pose_refine(_mvba._ptr(X), 300, pt_ptr.ctypes.data_as(i64), cam.ctypes.data_as(i32), _mvba._ptr(xy), len(cam), 8, None, None,
                                  None if K is None else _mvba._ptr(K), None if cams is None else cams.ctypes.data_as(i32),
                                  8 if cams is None else len(cams), n_steps, _mvba._ptr(R), _mvba._ptr(t), None, None, None, None, -1)
        return rc, lib.mvba_last_error().decode()

    for kw, text in (({"thr": 0.0}, "threshold = 0.0"), ({"thr": float("nan")}, "threshold = nan"), ({"thr": -0.5}, "threshold = -0.5"),
                     ({"H": 0}, "n_hypotheses = 0"), ({"H": 65537}, "n_hypotheses = 65537"), ({"n_refit": -1}, "n_refit = -1"),
                     ({"n_refit": 17}, "n_refit = 17"), ({"n_refine": -1}, "n_refine = -1"), ({"n_refine": 17}, "n_refine = 17"),
                     ({"cameras": [5, 8]}, "cameras[1] = 8"), ({"cameras": [-1]}, "cameras[0] = -1"), ({"nc": -1}, "n_cameras = -1"),
                     ({"nc": 3}, "n_cameras = 3 must be n_images = 8"), ({"K": None}, "null argument: K (argument 9)")):
        rc, msg = robust(**kw)
        assert rc == _mvba.MVBA_ERR_BADARG and text in msg, (kw, msg)
    for kw, text in (({"n_steps": -1}, "n_steps = -1"), ({"n_steps": 65}, "n_steps = 65"), ({"K": None}, "null argument: K (argument 10)"),
                     ({"cameras": [8]}, "cameras[0] = 8")):
        rc, msg = refine(**kw)
        assert rc == _mvba.MVBA_ERR_BADARG and text in msg, (kw, msg)


def test_pose_entry_points_fail_loudly_without_gpu():
    if os.path.exists(_mvba.LIB_PATH) and _mvba.device_count() > 0:
        pytest.skip("a device is visible")
    X, pt_ptr, cam, xy, K, _, _, _, _ = PC.case("300x8")
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        _mvba.pose_robust(X, pt_ptr, cam, xy, K, 0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        _mvba.pose_refine(X, pt_ptr, cam, xy, K, np.tile(np.eye(3), (8, 1, 1)), np.zeros((8, 3)))


def _premises(a, b, what, recorded_margin):
    """(a) the two routes give one result wherever a count table entry is not fragile, at most 1 % of a table is, and never a
    best hypothesis; (b) no distance within the recorded margin (relative, squared) of the threshold."""
    fr = PC.fragile(a, b)
    for key in ("status", "best", "n_inliers", "inlier", "n_usable", "sizes", "end"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    margin = min(a["margin"].min(), b["margin"].min())
    print(f"{what}: smallest |d^2 / thr^2 - 1| {margin:.3e} (recorded {recorded_margin:.1e}), fragile {fr.sum()} of {fr.size}")
    assert fr.sum() <= PC.FRAGILE_CAP * fr.size or fr.sum() == 0
    has = a["best"] >= 0
    assert not fr[np.nonzero(has)[0], a["best"][has]].any()
    assert recorded_margin <= margin <= 1.25 * recorded_margin and recorded_margin >= 1e-7


def _host_difference(a, b, what, recorded):
    ok = a["status"] == 0
    d = max(np.abs(a["R"][ok] - b["R"][ok]).max(), np.abs(a["t"][ok] - b["t"][ok]).max())
    dq = np.abs(a["quality"][ok] - b["quality"][ok]).max(axis=0)
    print(f"{what}: roots + chol vs ferrari + lstsq max |d(R, t)| = {d:.3e} (recorded {recorded:.1e}), RMS {dq[0]:.3e}, pivot {dq[1]:.3e}")
    assert 0.5 * recorded <= d <= recorded
    assert dq[0] <= PC.MARGIN * recorded
    R = a["R"][ok]
    np.testing.assert_allclose(R @ np.transpose(R, (0, 2, 1)), np.broadcast_to(np.eye(3), R.shape), rtol=0, atol=1e-13)
    assert (np.linalg.det(R) > 0).all()
    bad = ~ok
    assert np.isnan(a["R"][bad]).all() and np.isnan(a["t"][bad]).all() and np.isnan(a["quality"][bad]).all() and (a["n_inliers"][bad] == 0).all()


@pytest.mark.parametrize("name", sorted(PC.PARITY))
def test_parity_premises_and_host_versus_host_difference(name):
    a, b = PC.reference(name), PC.other(PC.reference, name)
    _premises(a, b, name, PC.POSE_MARGIN[name])
    _host_difference(a, b, name, PC.POSE_HOST_DIFF[name])
    if name == "300x8":  # without refits the result is the best hypothesis itself
        a0, b0 = PC.reference(name, n_refit=0), PC.other(PC.reference, name, n_refit=0)
        _host_difference(a0, b0, name + ", n_refit = 0", PC.POSE_HOST_DIFF["300x8_refit0"])
        np.testing.assert_array_equal(a0["n_inliers"], a0["hyp_count"].max(axis=1))
        assert (a0["quality"][:, 1] == 0).all()
        # the solutions a sample has: mostly two; a few per cent of the samples have none in front of the fourth point
        n_sol = np.bincount(a["n_sol"].ravel(), minlength=5)
        print("solutions per sample:", n_sol.tolist(), "degenerate:", (a["hyp_count"] < 0).mean())
        assert n_sol[2] > 0.8 * n_sol.sum() and n_sol[3] == 0 and 0 < (a["hyp_count"] < 0).mean() < 0.03


def test_reference_recovers_the_clean_observations():
    """30 % of every camera's observations replaced.  "coplanar_noisy" -- where the DLT is degenerate: the robust DLT reference has
    status 2 for all three cameras -- returns exactly the clean sets with R within 3e-3 of the truth; so do "edges_h65" and "dense";
    "300x8" does for seven cameras of eight (camera 1's best sample counts 117, one replaced observation within the threshold by
    chance; its first refit has 116 and is not kept: the rule as written)."""
    for name in ("coplanar_noisy", "edges_h65", "dense"):
        a, hit = PC.reference(name), np.asarray(PC.case(name)[8]).reshape(-1)
        assert (a["status"] == 0).all()
        np.testing.assert_array_equal(a["inlier"], ~hit, err_msg=name)
    X, pt_ptr, cam, xy, K, thr, H, seed, _ = PC.case("coplanar_noisy")
    assert (QR.resect_robust(X, pt_ptr, cam, xy, 3, thr, n_hyp=H, seed=seed)["status"] == 2).all()
    a, sc = PC.reference("coplanar_noisy"), PC.true_K("coplanar")[1]
    assert a["n_inliers"].tolist() == [55, 63, 55] and np.abs(a["R"] - sc.R_gt).max() < 3e-3
    a, hit = PC.reference("300x8"), PC.case("300x8")[8]
    assert a["n_inliers"].tolist() == [110, 117, 123, 99, 104, 105, 103, 102]
    assert (a["inlier"] & hit).sum() == 1 and a["sizes"][1].tolist() == [117, 116, -1] and a["end"][1] == "rejected"
    np.testing.assert_array_equal(a["inlier"] | hit, np.ones(len(hit), bool))


def test_exact_coplanar_data_gives_the_pose_to_rounding():
    X, pt_ptr, cam, xy, m, _ = IC.resect_case("coplanar")
    K, sc = PC.true_K("coplanar")
    a = PR.pose_robust(X, pt_ptr, cam, xy, K, PC.THRESHOLD, n_hyp=64, seed=1)
    assert (a["status"] == 0).all() and (a["n_inliers"] == a["n_usable"]).all()
    assert max(np.abs(a["R"] - sc.R_gt).max(), np.abs(a["t"] - sc.t_gt).max()) < 1e-12


def test_status_shapes_of_the_reference():
    for name in PC.STATUS_NAMES:
        a, b = PC.status_reference(name), PC.other(PC.status_reference, name)
        for key in ("hyp_count", "status", "best", "n_inliers", "inlier", "n_usable"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"{name}: {key}")
        assert min(a["margin"].min(), b["margin"].min()) >= 1e-4
        want = PC.status_case(name)[6]
        if want is not None:
            np.testing.assert_array_equal(a["status"], want, err_msg=name)
        if name != "collinear":
            _host_difference(a, b, name, PC.POSE_HOST_DIFF[name])
    r = PC.status_reference("four")
    assert r["n_usable"].tolist() == [60, 4, 3, 60] and (r["hyp_count"][1] == 4).all() and r["best"][1] == 0 and r["n_inliers"][1] == 4
    assert (r["hyp_count"][2] == -1).all() and r["best"][2] == -1
    r = PC.status_reference("collinear")
    assert (r["hyp_count"] == -1).all() and (r["best"] == -1).all() and not r["inlier"].any() and np.isnan(r["R"]).all()
    r = PC.status_reference("empty")
    assert (r["hyp_count"][list(IC.EMPTY_CAMERAS)] == -1).all() and (r["n_usable"][list(IC.EMPTY_CAMERAS)] == 0).all()
    a, b = PC.status_reference("point_ok"), PC.status_reference("nan_X")
    for key in ("R", "t", "quality", "hyp_count", "inlier", "n_usable", "n_inliers"):
        np.testing.assert_array_equal(a[key], b[key])
    assert (a["n_usable"] < PC.reference("300x8")["n_usable"]).all()
    # no geometry left in camera 3: every sample fits its own four observations and nothing else (status 0 with 4 inliers;
    # min_points is what keeps such a camera out of a reconstruction), a count of 3 where the fourth is beyond the threshold
    r = PC.status_reference("all_replaced")
    c = PC.ALL_REPLACED_CAMERA
    assert r["status"][c] == 0 and r["n_inliers"][c] == 4 and set(r["hyp_count"][c].tolist()) == {3, 4}


def test_refit_trace_of_the_reference():
    """"5000x3" at twice the noise: every kept refit moves the inlier set; at 16 the loop ends by rejection after 3."""
    for r in PC.REFIT_COUNTS:
        a, b = PC.refit_reference(r), PC.other(PC.refit_reference, r)
        _premises(a, b, f"refits, n_refit = {r}", PC.REFIT_MARGIN)
        _host_difference(a, b, f"refits, n_refit = {r}", PC.REFIT_HOST_DIFF[r])
        assert (a["n_accepted"] == a["n_changed"]).all()
    assert (PC.refit_reference(2)["n_accepted"] == 2).all()
    a = PC.refit_reference(16)
    assert a["n_accepted"].tolist() == [3, 3, 3] and (a["end"] == "rejected").all()
    s = a["sizes"]
    assert all(s[k, 4] < s[k, 3] for k in range(3))


def test_refine_reference():
    """From the ground truth perturbed by 1e-2 the iteration comes back to the noise level, never raises a camera's RMS, and ends
    by its own rule (a step that does not lower the cost) before the ten steps are used."""
    X, pt_ptr, cam, xy, K, R0, t0 = PC.refine_case()
    (Ra, ta, qa, nu, st), (Rb, tb, qb, _, _) = PC.refine_reference(), PC.refine_reference("lstsq")
    d = max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max())
    print(f"refine: chol vs lstsq {d:.3e} (recorded {PC.REFINE_HOST_DIFF:.1e}), RMS {qa[:, 0].max():.2e} -> {qa[:, 1].max():.2e}")
    assert 0.5 * PC.REFINE_HOST_DIFF <= d <= PC.REFINE_HOST_DIFF
    assert (st == 0).all() and (qa[:, 1] <= qa[:, 0]).all() and (qa[:, 1] < 1.6e-3).all() and (qa[:, 0] > 3e-3).all() and (qa[:, 2] < 10).all()
    sc = PC.true_K("300x8")[1]
    assert np.abs(Ra - sc.R_gt).max() < 2e-3 and np.abs(ta - sc.t_gt).max() < 1e-2
    np.testing.assert_array_equal(nu, np.bincount(cam, minlength=8))
    # n_steps = 0 leaves the poses alone; fewer than 3 observations: status 1; a NaN pose: status 2
    R1, t1, q1, _, s1 = PR.pose_refine(X, pt_ptr, cam, xy, K, R0, t0, n_steps=0)
    assert R1.tobytes() == R0.tobytes() and t1.tobytes() == t0.tobytes() and (q1[:, 0] == q1[:, 1]).all() and (q1[:, 2] == 0).all()
    few = np.zeros(len(cam), bool)
    few[np.nonzero(cam == 2)[0][:2]] = True
    few |= cam != 2
    tn = t0.copy()
    tn[5, 1] = np.nan
    R2, t2, q2, n2, s2 = PR.pose_refine(X, pt_ptr, cam, xy, K, R0, tn, obs_ok=few)
    assert s2.tolist() == [0, 0, 1, 0, 0, 2, 0, 0] and n2[2] == 2 and R2[2].tobytes() == R0[2].tobytes() and np.isnan(q2[[2, 5]]).all()


def test_camera_tiles():
    assert PC.camera_tile(300, 64) == 300 and PC.camera_tile(11, 65536) == 10 and PC.camera_tile(100, 512) == 100


def test_bootstrap_reference_on_contaminated_tracks():
    """20 % of the observations of cameras 2 .. 7 replaced: the calibrated registration reaches 8 cameras, keeps 251 points, uses
    no replaced observation, and its poses are within BOOT_FACTOR of the uncontaminated plain bootstrap's error -- in fact closer
    to the truth in R than that one."""
    sc, xy, hit = QC.bootstrap_case()
    (Ra, ta, Xa, ia), (Rb, tb, Xb, ib) = PC.reference_bootstrap(), PC.other(PC.reference_bootstrap)
    assert ia["order"] == ib["order"] and ia["camera_ok"].all() and len(ia["order"]) == 8
    for key in ("point_ok", "obs_ok", "inlier"):
        np.testing.assert_array_equal(ia[key], ib[key])
    ok = ia["point_ok"]
    d = max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max(), np.abs(Xa[ok] - Xb[ok]).max())
    clean = QC.plain_bootstrap(False)
    e_clean, e = QC.pose_error(sc, clean[0], clean[1], clean[3]["camera_ok"]), QC.pose_error(sc, Ra, ta, ia["camera_ok"])
    print(f"calibrated bootstrap: {ok.sum()} points, host difference {d:.3e} (recorded {PC.BOOT_HOST_DIFF:.1e}), pose error R {e[0]:.3e} "
          f"t {e[1]:.3e} (recorded {PC.BOOT_POSE_ERR}), uncontaminated R {e_clean[0]:.3e} t {e_clean[1]:.3e}")
    assert ok.sum() == 251
    assert 0.5 * PC.BOOT_HOST_DIFF <= d <= PC.BOOT_HOST_DIFF
    assert all(0.9 * r <= x <= r for x, r in zip(e, PC.BOOT_POSE_ERR))
    assert max(e) <= QC.BOOT_FACTOR * max(e_clean) and e[0] < e_clean[0]
    assert not (ia["inlier"] & hit).any() and not (ia["inlier"] & ~ia["obs_ok"]).any() and (hit & ~ia["obs_ok"]).sum() > 100
