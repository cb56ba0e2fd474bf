"""Calibrated robust resection, the part that needs no GPU: the sample generator libmvba.so exports is the
reference's and the first 4 draws of the two-view one, the argument checks, the premises under which the GPU parity tests may
ask for EXACT count tables (margins, fragile hypotheses), what the reference recovers, the host-versus-host figures that
tests/_pose_ransac_cases.py records, and -- from _limit_premises on -- the premises of the structural-limit cases of
tests/test_gpu_pose_limits.py, with what a deliberately wrong implementation would return on three of them."""
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


# ---- the structural limits ("Structural limits"): premises of tests/test_gpu_pose_limits.py ----
def _limit_premises(a, b, what):
    """_premises without the bracket of the margin: returns the smallest |d^2 / thr^2 - 1| of the two routes."""
    fr = PC.fragile(a, b)
    for key in ("status", "best", "n_inliers", "inlier", "n_usable", "sizes", "end", "n_accepted", "n_changed"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what}: {key}")
    assert fr.sum() <= PC.FRAGILE_CAP * fr.size
    has = a["best"] >= 0
    assert not fr[np.nonzero(has)[0], a["best"][has]].any()
    return min(a["margin"].min(), b["margin"].min()), int(fr.sum())


def _rt_difference(a, b):
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    return max(np.abs(a["R"] - b["R"]).max(), np.abs(a["t"] - b["t"]).max()), np.abs(a["quality"][:, 0] - b["quality"][:, 0]).max()


@pytest.mark.parametrize("name", sorted(PC.LIMITS))
def test_limit_premises_and_host_versus_host_difference(name):
    """Both routes give one table of integers at every n_refit the device runs, the smallest premise (b) and the case's host figure
    (a trace case: the largest over its n_refit with refits) are what tests/_pose_ransac_cases.py records."""
    counts = PC.LIMIT_REFIT_COUNTS if name in PC.TRACE_NAMES else (PC.LIMITS[name][5],)
    margin, worst = np.inf, 0.0
    for r in counts:
        a, b = PC.limit_reference(name, n_refit=r), PC.other(PC.limit_reference, name, n_refit=r)
        m, n_fragile = _limit_premises(a, b, f"{name}, n_refit = {r}")
        d, dq = _rt_difference(a, b)
        print(f"{name}, n_refit = {r}: smallest |d^2 / thr^2 - 1| {m:.3e}, fragile {n_fragile}, host |d(R, t)| {d:.3e}, RMS {dq:.3e}")
        margin = min(margin, m)
        assert dq <= PC.limit_margin(name, r)
        if r == 0:
            assert 0.5 * PC.LIMIT_REFIT0_DIFF <= d <= PC.LIMIT_REFIT0_DIFF
            np.testing.assert_array_equal(a["n_inliers"], a["hyp_count"].max(axis=1))
        else:
            worst = max(worst, d)
    rec_m, rec_d = PC.LIMIT_MARGIN[name], PC.LIMIT_HOST_DIFF[name]
    print(f"{name}: smallest premise (b) {margin:.3e} (recorded {rec_m:.1e}), host figure {worst:.3e} (recorded {rec_d:.1e})")
    assert rec_m <= margin <= 1.25 * rec_m and rec_m >= 1e-7
    assert 0.5 * rec_d <= worst <= rec_d


def test_limit_refit_traces():
    """The traces of "5000x3" at 16 refits that the device cases are built for: cameras of one tile that leave the loop at
    different refits; a fixed point kept for all 16 refits with the set unchanged; a kept refit that leaves the set as it is and is
    followed by a rejection; refits without a step (n_refine = 0), with one, with 16."""
    for name in PC.TRACE_NAMES:
        a = PC.limit_reference(name)
        got = [(int(n), int(c), str(e)) for n, c, e in zip(a["n_accepted"], a["n_changed"], a["end"])]
        assert got == PC.LIMIT_TRACES[name], (name, got)
    a = PC.limit_reference("refits_1.2e-3")
    assert len(set(a["n_accepted"].tolist())) == 3 and (a["n_accepted"] == a["n_changed"]).all()
    a = PC.limit_reference("refits_2.5e-3")
    assert a["sizes"][0, 4:].tolist() == [2915] * 13 and a["sizes"][0, 2:4].tolist() == [2914, 2914]
    assert a["sizes"][1, :5].tolist() == [2587, 2846, 2854, 2854, 2853]
    a = PC.limit_reference("refits_3e-3")
    assert a["sizes"][2, :5].tolist() == [2762, 2932, 2932, 2931, -1] and a["sizes"][0, 2:].tolist() == [3007] * 15
    # n_refine = 0: every refit is kept, none moves the pose or the set, no pivot is recorded
    a, a0 = PC.limit_reference("refine_0"), PC.limit_reference("refine_0", n_refit=0)
    assert a["R"].tobytes() == a0["R"].tobytes() and a["t"].tobytes() == a0["t"].tobytes() and (a["quality"][:, 1] == 0).all()
    assert (a["sizes"] == a["sizes"][:, :1]).all() and np.array_equal(a["inlier"], a0["inlier"])
    for name in ("refine_1", "refine_16"):  # (the hypotheses do not depend on n_refine)
        np.testing.assert_array_equal(PC.limit_reference(name)["hyp_count"], a["hyp_count"])
        assert (PC.limit_reference(name)["quality"][:, 1] > 1e-3).all()


def _refit_loop(name, k, accept=">=", read="current"):
    """A copy of the refit loop of _pose_ransac_ref.robust_pose_camera from the reference's best hypothesis of camera k on, with
    the two mask buffers of the device written out and two places open to a deliberate alteration: the accept rule (">=": kept
    while the set does not shrink) and the buffer the final mask is read from ("current"; "other": the one the last refit
    wrote, right only if that refit was kept).  Returns (n_inliers, mask)."""
    X, pt_ptr, cam, xy, K, thr, H, seed, n_refine, n_refit = PC.limit_case(name)
    pt = np.repeat(np.arange(len(X)), np.diff(pt_ptr))
    obs = np.nonzero(cam == k)[0]
    Xk, xk = X[pt[obs]], np.asarray(xy)[obs]
    idx = PR.sample(seed, k, int(PC.limit_reference(name)["best"][k]), len(Xk))[None]
    Rh, th, Ph, _ = PR.hypotheses(K[k], Xk[idx], xk[idx])
    d2, depth = QR.reprojection(Ph[0], Xk, xk)
    buf, cur, R, t = [(depth > 0) & (d2 <= thr * thr), None], 0, Rh[0], th[0]
    for _ in range(n_refit):
        Rr, tr, rec = PR.gauss_newton(K[k], R, t, Xk[buf[cur]], xk[buf[cur]], n_refine)
        assert rec["fail"] < 0
        d2, depth = QR.reprojection(PR.camera_matrix(K[k], Rr, tr), Xk, xk)
        buf[cur ^ 1] = (depth > 0) & (d2 <= thr * thr)
        kept = buf[cur ^ 1].sum() >= buf[cur].sum() if accept == ">=" else buf[cur ^ 1].sum() > buf[cur].sum()
        if not kept:
            break
        R, t, cur = Rr, tr, cur ^ 1
    mask = buf[cur] if read == "current" else buf[cur ^ 1]
    return int(mask.sum()), mask


def test_the_2_5e_3_trace_tells_a_wrong_refit_loop_from_a_right_one():
    """The copy as written reproduces the reference; with ">" for ">=" camera 0 stops at the first kept refit that leaves the
    count as it is (2914, not 2915); with the final mask read from the buffer the rejected refit wrote, camera 1 returns the
    rejected set (2853, not 2854).  Either changes n_inliers and the inlier bytes the device is asked for exactly."""
    name = "refits_2.5e-3"
    a, cam = PC.limit_reference(name), PC.limit_case(name)[2]
    for k in range(3):
        n, mask = _refit_loop(name, k)
        assert n == a["n_inliers"][k] and np.array_equal(mask, a["inlier"][cam == k])
    n, mask = _refit_loop(name, 0, accept=">")
    assert n == 2914 != a["n_inliers"][0] and not np.array_equal(mask, a["inlier"][cam == 0])
    n, mask = _refit_loop(name, 1, read="other")
    assert n == 2853 != a["n_inliers"][1] and not np.array_equal(mask, a["inlier"][cam == 1])
    assert _refit_loop(name, 1, accept=">")[0] == a["n_inliers"][1]  # (camera 1 alone would not tell the two rules apart)


def test_tiles_edges_premises_and_what_a_wrong_chunk_offset_would_return():
    """Four times the "edges" list at 65 536 hypotheses: two tiles, the second from entry 10 on, whose first chunk is 14.  A tile
    loop that put the second tile's chunk partials at the camera offset (10) would hand entries 10 and 11 other sums: the expected
    n_inliers change, so the case tells the two apart."""
    cams, H = list(PC.TILE_CAMERAS), PC.TILE_HYP
    a = PC.reference("edges_h65")
    tile, lc = PC.camera_tile(len(cams), H), PC.list_chunks(cams, a["n_usable"])
    assert tile == 10 and len(cams) == 12 and lc[10] == 14 != 10 and lc[-1] == 16 and a["n_usable"].tolist() == [257, 256, 255]
    cam = PC.case("edges_h65")[2]
    masks = [a["inlier"][cam == k] for k in range(3)]
    want = a["n_inliers"][cams]
    np.testing.assert_array_equal(PC.tile_sums(cams, a["n_usable"], masks, tile), want)
    wrong = PC.tile_sums(cams, a["n_usable"], masks, tile, offset="camera")
    assert (wrong[:10] == want[:10]).all() and (wrong[10:] != want[10:]).all()
    np.testing.assert_array_equal(PC.tile_sums(cams, a["n_usable"], masks, 12, offset="camera"), want)  # (one tile: nothing to tell)
    # the existing two-tile case has one chunk per entry: the wrong offset returns the right sums there
    b, c8 = PC.reference("300x8"), PC.case("300x8")[2]
    m8 = [b["inlier"][c8 == k] for k in range(8)]
    np.testing.assert_array_equal(PC.tile_sums([5] * 11, b["n_usable"], m8, 10, offset="camera"), b["n_inliers"][[5] * 11])


def test_general_K_is_the_plain_case_turned():
    """K' = 2.5 K Q: the camera matrices K' R'^T = 2.5 K R^T are those of "300x8" up to scale, so every integer is, t is, and
    R' = R Q -- within the host figure of the case."""
    a, p = PC.reference("300x8"), PC.limit_reference("general_K")
    K = PC.limit_case("general_K")[4]
    assert (np.abs(K) > 1e-3).all() and (np.abs(K[:, 2, 2] - 1.0) > 0.1).all() and (p["status"] == 0).all()
    firm = ~PC.fragile(a, PC.other(PC.reference, "300x8")) & ~PC.fragile(p, PC.other(PC.limit_reference, "general_K"))
    np.testing.assert_array_equal(a["hyp_count"][firm], p["hyp_count"][firm])
    for key in ("n_inliers", "best", "inlier", "n_usable", "sizes"):
        np.testing.assert_array_equal(a[key], p[key], err_msg=key)
    Q = PR.rodrigues(np.array(PC.Q_AXIS))
    dt, dR = np.abs(a["t"] - p["t"]).max(), np.abs(a["R"] @ Q - p["R"]).max()
    print(f"general_K: |t' - t| {dt:.3e} (recorded {PC.GENERAL_K_T_DIFF:.1e}), |R' - R Q| {dR:.3e} (recorded {PC.GENERAL_K_R_DIFF:.1e})")
    assert 0.5 * PC.GENERAL_K_T_DIFF <= dt <= PC.GENERAL_K_T_DIFF <= PC.LIMIT_HOST_DIFF["general_K"]
    assert 0.5 * PC.GENERAL_K_R_DIFF <= dR <= PC.GENERAL_K_R_DIFF <= PC.LIMIT_HOST_DIFF["general_K"]
    np.testing.assert_allclose(PR.camera_matrix(K, p["R"], p["t"]), PC.K_SCALE * PR.camera_matrix(PC.case("300x8")[4], a["R"], a["t"]),
                               rtol=0, atol=50 * PC.LIMIT_HOST_DIFF["general_K"])  # (|K'| <= 5, |t| <= 10)


def _refine_difference(name):
    A, B = PC.refine_limit_reference(name), PC.refine_limit_reference(name, "lstsq")
    np.testing.assert_array_equal(A[4], B[4])
    np.testing.assert_array_equal(A[3], B[3])
    ok = A[4] == 0
    d = max(np.abs(A[0][ok] - B[0][ok]).max(), np.abs(A[1][ok] - B[1][ok]).max())
    print(f"refine {name}: chol vs lstsq {d:.3e}, steps {A[2][:, 2].tolist()} / {B[2][:, 2].tolist()}")
    return A, B, d


@pytest.mark.parametrize("name", sorted(PC.REFINE_LIMIT_HOST_DIFF))
def test_refine_limit_host_versus_host_difference(name):
    A, B, d = _refine_difference(name)
    rec = PC.REFINE_LIMIT_HOST_DIFF[name]
    assert 0.5 * rec <= d <= rec
    ok = A[4] == 0
    assert np.abs(A[2][ok, :2] - B[2][ok, :2]).max() <= PC.MARGIN * rec and (A[2][ok, 1] <= A[2][ok, 0]).all()


def test_refine_step_count_premises():
    """n_steps = 1 and 2: both routes take exactly 1 and 2 steps with every camera -- the last permitted step is accepted -- and
    still lower the cost; at 64 the iteration ends by its own rule after 3 .. 6 steps."""
    for n in (1, 2):
        for solver in ("chol", "lstsq"):
            q = PC.refine_limit_reference(f"steps_{n}", solver)[2]
            assert (q[:, 2] == n).all() and (q[:, 1] < q[:, 0]).all()
    q1, q2 = PC.refine_limit_reference("steps_1")[2], PC.refine_limit_reference("steps_2")[2]
    assert (q2[:, 1] < q1[:, 1]).all()
    for solver in ("chol", "lstsq"):
        q = PC.refine_limit_reference("steps_64", solver)[2]
        assert (q[:, 2] >= 3).all() and (q[:, 2] <= 6).all()
    assert PC.refine_limit_reference("steps_64")[2][:, 2].tolist() == [4, 5, 3, 3, 3, 3, 4, 3]


def test_refine_mask_premises_and_what_a_wrong_mask_index_would_return():
    """obs_ok by chunk of each camera's run: 20 chunks per camera cycling all / none / lane 255 alone / a seeded half, the last
    of 136 observations; with point_ok the runs shrink to about 3500 and both masks act together.  An implementation that read
    the byte at the observation's place in the sorted run instead of its place in the caller's list would use other
    observations: n_usable changes, so the case tells the two apart."""
    for name in ("masks", "masks_point_ok"):
        X, pt_ptr, cam, xy, K, R0, t0, ok, obs_ok, n_steps = PC.refine_limit_case(name)
        pt = np.repeat(np.arange(len(X)), np.diff(pt_ptr))
        usable = np.ones(len(cam), bool) if ok is None else ok[pt]
        for k in range(3):
            run = np.nonzero((cam == k) & usable)[0]
            per = [int(obs_ok[run[i: i + 256]].sum()) for i in range(0, len(run), 256)]
            if name == "masks":
                assert len(run) == 5000 and len(per) == 20 and len(run) - 19 * 256 == 136
            else:
                assert 3400 < len(run) < 3600 and len(per) == 14 and not obs_ok[(cam == k) & ~usable].any()
            assert per[0::4] == [256] * len(per[0::4]) and per[1::4] == [0] * len(per[1::4]) and per[2::4] == [1] * len(per[2::4])
            assert all(obs_ok[run[i + 255]] for i in range(512, len(run) - 255, 1024)) and all(0.35 * 256 < c < 0.65 * 256 for c in per[3::4][:-1])
            if name == "masks":  # the last chunk is partial and of the fourth kind (with point_ok it is of the second: nothing)
                assert 0 < per[-1] < 136
        A = PC.refine_limit_reference(name)
        assert A[3].tolist() == PC.MASK_USABLE[name] == [int((obs_ok & usable & (cam == k)).sum()) for k in range(3)] and (A[4] == 0).all()
        order = np.argsort(cam, kind="stable")  # the sorted list: camera-major, ascending points
        wrong = np.zeros(len(cam), bool)
        wrong[order] = obs_ok  # the observation at sorted position i gets the byte of the caller's position i
        W = PR.pose_refine(X, pt_ptr, cam, xy, K, R0, t0, point_ok=ok, obs_ok=wrong, n_steps=n_steps)
        assert (W[3] != A[3]).all(), (W[3], A[3])


def test_refine_status_premises():
    """Exact data at the ground truth.  Call a: everything (status 0), the 40 collinear points (the first normal matrix fails
    the pivot rule: status 2), three collinear points (status 2).  Call b: three points off the line (status 0 at the minimum),
    two points (status 1).  The failing pivots are below 1e-14 or negative, the passing one of the minimum far above 1e-12."""
    for solver in ("chol", "lstsq"):
        A, B = PC.refine_limit_reference("statuses_a", solver), PC.refine_limit_reference("statuses_b", solver)
        assert A[4].tolist() == PC.STATUS_WANT["statuses_a"] and A[3].tolist() == [80, 40, 3]
        assert B[4].tolist() == PC.STATUS_WANT["statuses_b"] and B[3].tolist() == [80, 3, 2] and B[5][2] is None
        fp = [A[5][k]["fail_pivot"] for k in (1, 2)]
        print(f"statuses ({solver}): failing relative pivots {fp[0]:.3e}, {fp[1]:.3e}; the three-observation camera's smallest {B[5][1]['pivot']:.3e}")
        assert all(A[5][k]["fail"] == 0 for k in (1, 2)) and A[5][0]["fail"] == B[5][0]["fail"] == B[5][1]["fail"] == -1
        assert 0 < fp[0] < PC.STATUS_PIVOT_BOUND and 0.5 * PC.STATUS_FAIL_PIVOT <= fp[0] <= PC.STATUS_FAIL_PIVOT and fp[1] < 0
        assert 0.9 * PC.STATUS_MIN_PIVOT <= B[5][1]["pivot"] <= 1.1 * PC.STATUS_MIN_PIVOT
        R0, t0 = PC.refine_limit_case("statuses_a")[5:7]
        for out in (A, B):  # a camera of status != 0 keeps its pose, NaN quality
            bad = out[4] != 0
            assert out[0][bad].tobytes() == np.ascontiguousarray(R0[bad]).tobytes() and np.isnan(out[2][bad]).all() and np.isfinite(out[2][~bad]).all()
    X = PC.refine_limit_case("statuses_a")[0]
    assert np.linalg.matrix_rank(X[:40] - X[0], tol=1e-12) == 1 and np.linalg.matrix_rank(X[40:43] - X[40], tol=1e-6) == 2
    A = PC.refine_limit_reference("empty")
    assert A[4].tolist() == [0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1] and (A[3][[1, 4, 10]] == 0).all()
    full = PC.refine_reference()
    assert A[0][A[4] == 0].tobytes() == full[0].tobytes() and A[1][A[4] == 0].tobytes() == full[1].tobytes()


def test_guards_that_no_case_reaches():
    """A pivot failure at a later step (PG_FAIL = j > 0) and a solver failure inside a pose refit (end == "solver") are reached by
    no case of this file, on either route; none was built."""
    for solver in ("chol", "lstsq"):
        for name in PC.REFINE_LIMIT_NAMES:
            assert all(r is None or r["fail"] <= 0 for r in PC.refine_limit_reference(name, solver)[5]), name
    ends = []
    for name in PC.LIMITS:
        for r in (PC.LIMIT_REFIT_COUNTS if name in PC.TRACE_NAMES else (2,)):
            ends += [PC.limit_reference(name, n_refit=r)["end"], PC.other(PC.limit_reference, name, n_refit=r)["end"]]
    ends += [PC.reference(name)["end"] for name in PC.PARITY] + [PC.refit_reference(r)["end"] for r in PC.REFIT_COUNTS]
    assert not (np.concatenate(ends) == "solver").any()
