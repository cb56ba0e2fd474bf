"""Planar scenes, the part that needs no GPU: the sample generator and the entry points libmvba.so exports, the
decomposition of a calibrated homography, the premises under which the GPU parity tests may ask for EXACT integers, what the
reference recovers from contaminated planar pairs, the selection ratios, and the host-versus-host differences that set the GPU
margins -- all of them what tests/_homography_cases.py records."""
import ctypes
import os

import numpy as np
import pytest

import _homography_cases as HC
import _homography_ref as HR
import _ransac_cases as RC
import _twoview_cases as C
import _twoview_ref as T
from lib import _mvba
from lib.initialization import homography_pose_candidates, homography_sample, ransac_sample

SAMPLE_TABLE = [(0, 0, 1, 0, 4), (1, 0, 1, 5, 80), (1, 0, 1, 511, 80), ((1 << 64) - 1, 3, 2, 7, (1 << 31) - 1), (7, 5, 2, 511, 300),
                (1, 1703, 0, 65535, 5), (12345678901234567890, 6, 7, 3, 8), (1, 1, 0, 5, 7)]


@pytest.mark.parametrize("seed,k,l,h,n", SAMPLE_TABLE)
def test_exported_sample_generator_is_the_reference(seed, k, l, h, n):
    """n = 4 (a permutation), n below 8 (which mvba_ransac_sample refuses), n = 2^31 - 1, k > l, seed = 2^64 - 1; and for n >= 8 the
    first four draws of the 8-point sampler."""
    got, want = homography_sample(seed, k, l, h, n), HR.sample(seed, k, l, h, n)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int64 and len(set(got.tolist())) == 4 and (got >= 0).all() and (got < n).all()
    if n == 4:
        assert sorted(got.tolist()) == [0, 1, 2, 3]
    if n >= 8:
        np.testing.assert_array_equal(got, ransac_sample(seed, k, l, h, n)[:4])


def test_sample_rejects_bad_arguments():
    with pytest.raises(ValueError, match="n = 3"):
        homography_sample(0, 0, 1, 0, 3)
    with pytest.raises(ValueError, match="h = -1"):
        homography_sample(0, 0, 1, -1, 80)
    with pytest.raises(ValueError, match="must be in 4"):
        homography_sample(0, 0, 1, 0, 1 << 31)


def test_library_exports_the_homography_entry_points():
    """The new symbols exist with bound prototypes; argument errors come before any device work and name the number."""
    names = ("mvba_homography_robust", "mvba_homography_sample")
    for name in names:
        assert name in _mvba.SIGNATURES, name
    raw = ctypes.CDLL(_mvba.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), name
    lib = _mvba.load_library()
    for name in names:
        res, args = _mvba.SIGNATURES[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args
    i32, i64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    pt_ptr, cam, xy, m, _, _, _, _, _, _ = HC.case("planar80x3")
    xy = np.ascontiguousarray(xy)
    Hm, pairs = np.empty((1, 9)), np.array([(0, 1)], np.int32)

    def call(thr=0.01, H=16, n_refit=2, pair=(0, 1), out=Hm):
        pairs[0] = pair
        rc = lib.mvba_homography_robust(80, m, pt_ptr.ctypes.data_as(i64), cam.ctypes.data_as(i32), _mvba._ptr(xy), len(cam), pairs.ctypes.data_as(i32),
                                        1, thr, H, 1, n_refit, None if out is None else _mvba._ptr(out), None, None, None, None, None, None, None, None, -1)
        return rc, lib.mvba_last_error().decode()

    for kw, text in (({"thr": 0.0}, "threshold = 0.0"), ({"thr": float("nan")}, "threshold = nan"), ({"thr": -0.5}, "threshold = -0.5"),
                     ({"H": 0}, "n_hypotheses = 0"), ({"H": 65537}, "n_hypotheses = 65537"), ({"n_refit": -1}, "n_refit = -1"),
                     ({"n_refit": 17}, "n_refit = 17"), ({"pair": (2, 2)}, "(2, 2)"), ({"pair": (2, 3)}, "n_images = 3"),
                     ({"out": None}, "null argument: H (argument 13)")):
        rc, msg = call(**kw)
        assert rc == _mvba.MVBA_ERR_BADARG and text in msg, (kw, msg)


def test_homography_robust_fails_loudly_without_gpu():
    if os.path.exists(_mvba.LIB_PATH) and _mvba.device_count() > 0:
        pytest.skip("a device is visible")
    pt_ptr, cam, xy, m, pairs = HC.case("planar80x3")[:5]
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        _mvba.homography_robust(pt_ptr, cam, xy, m, pairs, 0.01)


def test_pose_candidates_contain_the_ground_truth():
    """Hn = R^T (I + t n^T / d) built from the ground truth of the planar scene (d in units of the baseline): one of the four
    candidates is the truth to rounding, with the plane; the library's and the reference's lists agree, by both routes."""
    sc, X, _ = HC.planar_scene(80, 3, 0)
    for k, l in ((0, 1), (1, 2), (2, 0)):
        Rg, tg = C.true_relative_pose(sc, k, l)
        base = np.linalg.norm(sc.t_gt[l] - sc.t_gt[k])
        n_w = np.array([1.0, 0.0, 0.0])  # the plane x = 0 of the world
        n_k = sc.R_gt[k].T @ n_w
        d = -(n_w @ sc.t_gt[k]) / base  # n_k . X_k = d for points of the plane, in units of the baseline
        if d < 0:
            n_k, d = -n_k, -d
        Hn = Rg.T @ (np.eye(3) - np.outer(tg, n_k) / d)  # x_l ~ R^T (X - t) with n . X = d: X - t = (I - t n^T / d) X
        Xk = (X - sc.t_gt[k]) @ sc.R_gt[k] / base
        xk, xl = Xk[:, :2] / Xk[:, 2:], None
        Xl = (Xk - tg) @ Rg
        np.testing.assert_allclose(np.c_[xk, np.ones(80)] @ Hn.T / (np.c_[xk, np.ones(80)] @ Hn[2])[:, None], Xl / Xl[:, 2:], atol=1e-12)
        for scale in (1.0, -3.7):  # any scale and sign of Hn
            cands = homography_pose_candidates(scale * Hn)
            assert len(cands) == 4
            i, err = HR.closest_candidate(cands, Rg, tg)
            nn = cands[i][2]
            perr = max(np.abs(nn / np.linalg.norm(nn) - n_k).max(), abs(1.0 / np.linalg.norm(nn) - d))
            print(f"pair ({k}, {l}) scale {scale}: candidate {i} is the truth to {err:.2e}, its plane to {perr:.2e}")
            assert err <= 1e-12 and perr <= 1e-12
            for route in ("eigh", "svd"):
                for a, b in zip(cands, HR.pose_candidates(scale * Hn, route)):
                    assert max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max(), np.abs(a[2] - b[2]).max()) <= 1e-11
            assert all(abs(np.linalg.det(R) - 1.0) <= 1e-12 and abs(np.linalg.norm(t) - 1.0) <= 1e-12 for R, t, _ in cands)
            np.testing.assert_array_equal(cands[0][1], -cands[1][1])
            np.testing.assert_array_equal(cands[2][2], -cands[3][2])


def test_pose_candidates_of_a_pure_rotation_are_none():
    sc = HC.planar_scene(80, 3, 0)[0]
    Rrel = sc.R_gt[1].T @ sc.R_gt[0]
    assert homography_pose_candidates(Rrel) == [] and homography_pose_candidates(-2.5 * Rrel) == [] and HR.pose_candidates(Rrel) == []
    assert homography_pose_candidates(np.full((3, 3), np.nan)) == [] and homography_pose_candidates(np.zeros((3, 3))) == []


def _premises(a, b, what):
    """(a) the two routes give one count table and one of every other integer; (b) no test within GUARD of its threshold;
    (c) no sample within a factor 100 of the degeneracy rule."""
    np.testing.assert_array_equal(a["hyp_count"], b["hyp_count"])
    for key in ("status", "best", "n_inliers", "inlier", "n_shared", "n_accepted", "end"):
        np.testing.assert_array_equal(a[key], b[key])
    guard = min(a["margin"].min(), b["margin"].min())
    piv = a["pivot"][np.isfinite(a["pivot"])]
    near = (piv > 1e-14) & (piv < 1e-10)
    print(f"{what}: guard {guard:.2e}, sample pivots in {piv.min() if len(piv) else np.nan:.2e} .. {piv.max() if len(piv) else np.nan:.2e}")
    assert guard >= HC.GUARD and not near.any()
    # a sample fits its own 4 points, but a point whose third coordinate is negative is no inlier: counts below 4 do occur (the
    # horizon of the hypothesis between the sample and the centroid).  Status 4 needs EVERY hypothesis to be of that kind: H = 1.
    best = a["hyp_count"].max(axis=1)
    np.testing.assert_array_equal(a["status"] == 4, (best >= 0) & (best < 4))


def _host_diff(a, b, name, exact_fit=False):
    """``exact_fit``: every inlier is fitted to rounding (four points, or no noise) -- the RMS is rounding itself, compared with
    the size of the coordinates (1) instead of its own."""
    ok = a["status"] == 0
    d = np.abs(a["H"][ok] - b["H"][ok]).max()
    rel = (np.abs(a["quality"][ok, 0] - b["quality"][ok, 0]) / (1.0 if exact_fit else a["quality"][ok, 0])).max()
    dr = np.abs(a["quality"][ok, 1] - b["quality"][ok, 1]).max()
    print(f"{name}: closed form / eigh vs SVD max |dH| = {d:.3e} (recorded {HC.HOST_DIFF[name]:.1e}), RMS relative {rel:.3e}, ratio {dr:.3e}")
    assert 0.5 * HC.HOST_DIFF[name] <= d <= HC.HOST_DIFF[name]
    assert rel <= HC.MARGIN * HC.HOST_DIFF[name] and dr <= HC.MARGIN * HC.HOST_DIFF[name]
    Hm = a["H"][ok].reshape(-1, 9)
    np.testing.assert_allclose(np.linalg.norm(Hm, axis=1), 1.0, rtol=0, atol=1e-14)
    assert (Hm[np.arange(len(Hm)), np.abs(Hm).argmax(axis=1)] > 0).all()


@pytest.mark.parametrize("name", sorted(HC.PARITY))
def test_parity_premises_and_host_versus_host_difference(name):
    a, b = HC.reference(name), HC.reference(name, "svd")
    _premises(a, b, name)
    assert (a["status"] == 0).all()
    _host_diff(a, b, name)
    _premises(HC.reference(name, "closed", 0), HC.reference(name, "svd", 0), name + ", n_refit = 0")


def test_limit_premises_and_host_versus_host_differences():
    """Every structural-limit case of test_gpu_homography.py: statuses, premises, recorded figures."""
    a, b = HC.mixed_reference(), HC.mixed_reference("svd")
    _premises(a, b, "mixed")
    np.testing.assert_array_equal(a["status"], HC.mixed_case()[5])
    assert a["n_shared"].tolist() == [80, 3, 80, 80, 3, 80, 80, 80, 3]
    _host_diff(a, b, "mixed")
    for H in (1, 64, 65):
        a, b = HC.reference("planar80x3", n_hyp=H), HC.reference("planar80x3", "svd", n_hyp=H)
        _premises(a, b, f"H = {H}")
        _host_diff(a, b, f"h{H}")
        # one hypothesis alone: two of the four pairs draw one that counts fewer than its own four points -- status 4 from data
        assert a["status"].tolist() == ([0, 0, 4, 4] if H == 1 else [0, 0, 0, 0])
    best = [HC.reference("planar80x3", n_hyp=H)["best"].tolist() for H in (64, 65)]
    print("best at H = 64, 65:", best)
    # exactly four shared points: every hypothesis is a permutation of them, all counts are 4, the refit is the DLT of 4 points
    pt_ptr, cam, xy, m, pairs = HC.few_case(4)
    a, b = (HR.homography_robust(pt_ptr, cam, xy, m, pairs, HC.THRESHOLD, 64, 2, 2, r) for r in ("closed", "svd"))
    _premises(a, b, "four")
    assert a["status"].tolist() == [0] and (a["hyp_count"] == 4).all() and a["best"][0] == 0 and a["n_inliers"][0] == 4
    _host_diff(a, b, "four", exact_fit=True)
    pt_ptr, cam, xy, m, pairs = HC.few_case(3)
    a = HR.homography_robust(pt_ptr, cam, xy, m, pairs, HC.THRESHOLD, 64, 2, 2)
    assert a["status"].tolist() == [1] and (a["hyp_count"] == -1).all() and a["n_shared"][0] == 3
    # the refits: pairs leave the loop at different refits, and the inlier sets move
    worst = 0.0
    for r in HC.REFIT_COUNTS:
        a, b = HC.refit_reference(r), HC.refit_reference(r, "svd")
        _premises(a, b, f"refits, n_refit = {r}")
        worst = max(worst, np.abs(a["H"] - b["H"]).max())
    a = HC.refit_reference(16)
    print("refits at 16:", list(zip(a["n_accepted"].tolist(), a["n_changed"].tolist(), a["end"].tolist())), f"host figure {worst:.3e}")
    assert len(set(RC.end_refit(a, 16).tolist())) >= 2 and a["n_changed"].max() >= 2
    assert 0.5 * HC.HOST_DIFF["refits"] <= worst <= HC.HOST_DIFF["refits"]
    # the noise-free plane: every hypothesis is the exact H, both ways round, and the two are inverses of each other
    pt_ptr, cam, xy, m, pairs = HC.noise_free_case()
    a, b = (HR.homography_robust(pt_ptr, cam, xy, m, pairs, HC.THRESHOLD, 16, 1, 2, r) for r in ("closed", "svd"))
    assert (a["status"] == 0).all() and (a["hyp_count"] == 80).all() and (b["hyp_count"] == 80).all()
    _host_diff(a, b, "noise_free", exact_fit=True)
    inv = HR.unit(np.linalg.inv(a["H"][0]))
    assert np.abs(inv - a["H"][1]).max() <= HC.MARGIN * HC.HOST_DIFF["noise_free"]
    # H = 65 536: the sampled entries of the count table
    for which in ("four", "eighty"):
        hs, c, guard, pivot = HC.max_hyp_reference(which)
        c2, guard2 = HC.max_hyp_reference(which, "svd")[1:3]
        np.testing.assert_array_equal(c, c2)
        print(f"max hyp, {which}: guard {min(guard, guard2):.2e}, degenerate {int((c < 0).sum())} of {len(hs)}")
        assert min(guard, guard2) >= HC.GUARD and len(hs) == 739 and not ((pivot > 1e-14) & (pivot < 1e-10)).any()


def test_reference_recovers_exactly_the_clean_points():
    """"planar80x3" pair (1, 2), 30 % of image 2 replaced: the final inliers are exactly the clean shared points, and the refit IS
    the fit of the clean points."""
    pt_ptr, cam, xy, m, pairs, thr, H, seed, bad, _ = HC.case("planar80x3")
    a = HC.reference("planar80x3")
    i = [tuple(p) for p in pairs].index((1, 2))
    ids, xk, xl = T.shared(pt_ptr, cam, np.asarray(xy), 1, 2)
    assert len(ids) == 80 and bad.sum() == 24 and a["n_inliers"][i] == 56
    np.testing.assert_array_equal(a["inlier"][i][ids], ~bad)
    np.testing.assert_array_equal(a["H"][i], HR.homography(xk[~bad], xl[~bad])[0])
    plain = HR.homography(xk, xl)[0]
    print(f"planar80x3 (1, 2): the plain fit of all 80 is {np.abs(plain - a['H'][i]).max():.2f} from the clean H")
    assert np.abs(plain - a["H"][i]).max() > 0.05


def test_homography_pose_is_closer_to_the_truth_than_the_eight_point_pose():
    """The contaminated pair (1, 2): the reference's homography pose against the truth, and the 8-point pose of the UNcontaminated
    pair (status 0: with noise the pivot rule passes), which is wrong without saying so."""
    R, t, X, info = HC.reference_pose()
    R2, t2, _, _ = HC.reference_pose(route="svd")
    Rg, tg = HC.true_pose("planar80x3", 1, 2)
    sc, _, xy = HC.planar_scene(80, 3, 0)
    R8, t8, _, i8 = T.relative_pose(sc.pt_ptr, sc.cam_idx, xy, sc.K_gt, (1, 2))
    eh, e8, hd = HC.pose_error(R, t, Rg, tg), HC.pose_error(R8, t8, Rg, tg), max(np.abs(R - R2).max(), np.abs(t - t2).max())
    print(f"pose error: homography {eh:.3e} (recorded {HC.POSE_H_ERR:.1e}), 8-point on clean data {e8:.3e} (recorded {HC.POSE_F8_ERR:.1e}, status "
          f"{i8['status']}), host-versus-host {hd:.2e} (recorded {HC.POSE_HOST_DIFF:.1e}); n_front {info['n_front']}, ambiguous {info['ambiguous']}")
    assert info["status"] == 0 and i8["status"] == 0 and info["model"] == "homography" and not info["ambiguous"]
    assert info["n_front"].max() == 56 and info["n_inliers"] == 56 and np.isfinite(X).all(axis=1).sum() == 56
    assert 0.8 * HC.POSE_H_ERR <= eh <= HC.POSE_H_ERR and 0.8 * HC.POSE_F8_ERR <= e8 <= 1.25 * HC.POSE_F8_ERR
    assert HC.POSE_FACTOR * eh <= e8 and 0.5 * HC.POSE_HOST_DIFF <= hd <= HC.POSE_HOST_DIFF
    n_k, d = info["plane"]
    assert abs(np.linalg.norm(n_k) - 1.0) <= 1e-12 and d > 0


def test_auto_selection_ratios():
    """model="auto": the homography on the planar pairs, the fundamental matrix on the general scenes; the ratios are the recorded
    ones and planar_ratio = 0.8 lies between the two groups.  The contaminated grazing pair is below it: the recorded limit."""
    for (name, pair), want in HC.RATIO_PLANAR.items():
        pt_ptr, cam, xy, m, _, thr, H, seed, _, K = HC.case(name)
        info = HR.relative_pose(pt_ptr, cam, xy, K, pair, thr, "auto", n_hyp=H, seed=seed)[3]
        print(f"{name} {pair}: n_inliers_H / n_inliers_F = {info['ratio']:.3f} (recorded {want}), model {info['model']}")
        assert info["model"] == "homography" and abs(info["ratio"] - want) <= 5e-4 and info["status"] == 0
    for name, want in HC.RATIO_GENERAL.items():
        info = HC.general_pose(name)[3]
        print(f"{name} (0, 1): ratio {info['ratio']:.3f} (recorded {want}), model {info['model']}")
        assert info["model"] == "fundamental" and abs(info["ratio"] - want) <= 5e-4 and info["status"] == 0
    assert max(HC.RATIO_GENERAL.values()) < 0.8 < min(HC.RATIO_PLANAR.values())
    pt_ptr, cam, xy, m, _, thr, H, seed, _, K = HC.case("planar80x3")
    info = HR.relative_pose(pt_ptr, cam, xy, K, (0, 2), thr, "auto", n_hyp=H, seed=seed)[3]
    assert abs(info["ratio"] - HC.RATIO_GRAZING) <= 5e-4 and info["model"] == "fundamental"


def test_altered_copies_change_the_expected_integers():
    """The cases can tell: a transfer tested one way only, and the degeneracy rule removed, each change an integer output."""
    a = HC.reference("planar80x3")
    one = HC.reference("planar80x3", one_way=True)
    assert not np.array_equal(a["hyp_count"], one["hyp_count"]) and (one["hyp_count"] >= a["hyp_count"]).all()
    print("one-way test: hypothesis counts differ in", int((a["hyp_count"] != one["hyp_count"]).sum()), "entries; n_inliers", a["n_inliers"], "->",
          one["n_inliers"])
    ptr, cam, xy, m, pairs, want = HC.mixed_case()
    loose = HR.homography_robust(ptr, cam, xy, m, pairs, HC.THRESHOLD, 64, 2, 2, no_degeneracy_rule=True)
    b = HC.mixed_reference()
    deg = want == 2
    assert (b["hyp_count"][deg] == -1).all() and not np.array_equal(loose["hyp_count"][deg], b["hyp_count"][deg])
    assert not np.array_equal(loose["status"], b["status"])


def test_reference_bootstrap_on_the_planar_scene():
    """The planar 300 x 8 twin, 20 % of cameras 2 .. 7 replaced: the reference registers all 8 cameras from a homography start and
    uses no replaced observation.  (X[:, 1] = 0 finds no start pair of status 0 and X[:, 2] = 0 admits one replaced observation:
    X[:, 0] = 0 is the scene for which the premise holds.)"""
    sc, X, xy, hit = HC.bootstrap_case()
    R, t, Xr, info = HC.reference_bootstrap()
    assert info["model"] == "homography" and info["camera_ok"].all() and len(info["order"]) == 8
    assert not (info["inlier"] & hit).any()
    print(f"planar bootstrap: order {info['order']}, {info['point_ok'].sum()} points, ambiguous start {info['ambiguous']}")


def test_reference_bootstrap_from_an_ambiguous_start():
    """The same scene without the shared points of pair (0, 1) that the second candidate's plane puts behind camera 0: two
    candidates put all 33 inliers in front, the start is ``ambiguous``, and the driver runs under both.  On this scene the first
    registered camera has the same 14 inliers under either (a calibrated camera can be resected against the wrong plane's points
    too, when they are few): the tie keeps the first, the candidate with the lower triangulation RMS, and that is the true one."""
    from lib.initialization import engine_intrinsics

    sc, ptr, cam, xy, hit, _ = HC.ambiguous_case()
    info = HR.homography_pose(ptr, cam, xy, engine_intrinsics(sc.init_K), (0, 1), HC.THRESHOLD, 512, 1)[3]
    top = np.sort(info["n_front"])[::-1]
    assert info["ambiguous"] and top[0] == top[1] == info["n_inliers"] == 33 and top[2] == 0
    R, t, X, bi = HC.ambiguous_reference()
    Rg = sc.R_gt[0].T @ sc.R_gt[1]
    print(f"ambiguous start: order {bi['order']}, |R_1 - truth| = {np.abs(R[1] - Rg).max():.3e}, {bi['point_ok'].sum()} points")
    assert bi["ambiguous"] and bi["model"] == "homography" and bi["camera_ok"].all() and not (bi["inlier"] & hit).any()
    assert np.abs(R[1] - Rg).max() <= 2e-2  # (the other candidate's R_1 is 0.91 away)


def test_arithmetic_of_the_ambiguous_start_round():
    """The three helpers bootstrap's ambiguous-start branch decides by, in all three forms of the registration round (inliers of
    the robust forms, usable observations of the plain one): they need no device."""
    from lib.initialization import _other_start_wins, _registration_count, _usable_counts

    st, cnt = np.array([0, 2, 0, 0, 4]), np.array([11, 90, 14, 13, 80])
    assert _registration_count(st, cnt, 12) == 14 and _registration_count(st, cnt, 15) == 0 and _registration_count(st, cnt, 1) == 14
    assert _registration_count(np.array([1, 2]), np.array([50, 60]), 12) == 0 and _registration_count(np.zeros(0, int), np.zeros(0, int), 12) == 0
    assert _registration_count([0], [12], 12) == 12
    assert _other_start_wins(14, 15, 0) and not _other_start_wins(14, 14, 0) and not _other_start_wins(14, 13, 0)
    assert not _other_start_wins(14, 99, 3) and not _other_start_wins(0, 0, 0)
    sc, ptr, cam, xy, _, _ = HC.ambiguous_case()
    ok = np.random.default_rng(5).random(len(ptr) - 1) < 0.4
    pt = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    want = np.array([int((ok[pt] & (cam == c)).sum()) for c in range(9)])  # (a ninth camera that sees nothing)
    np.testing.assert_array_equal(_usable_counts(ptr, cam, ok, 9), want)
    assert want[8] == 0 and _usable_counts(ptr, cam, np.zeros(len(ptr) - 1, bool), 8).tolist() == [0] * 8
