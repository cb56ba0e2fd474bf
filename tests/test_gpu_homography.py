"""Planar scenes on the device: mvba_homography_robust against the NumPy restatement of tests/_homography_ref.py
-- integers exactly (the premises are asserted by test_homography_cpu.py), H and quality within MARGIN x the recorded
host-versus-host figure --, its structural limits, relative_pose and bootstrap with ``model``, and the fundamental matrix through
the loop the two fits now share."""
import numpy as np
import pytest

import _homography_cases as HC
import _homography_ref as HR
import _ransac_cases as RC
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster
from lib.initialization import bootstrap, relative_pose, restrict_observations, robust_fundamental_matrices, robust_homographies

pytestmark = pytest.mark.gpu

KEYS = ("H", "quality", "n_shared", "n_inliers", "best", "status", "inlier", "hyp_count")


def _run(pt_ptr, cam, xy, m, pairs, thr, H, seed, n_refit=2):
    return _mvba.homography_robust(pt_ptr, cam, xy, m, pairs, thr, n_hypotheses=H, seed=seed, n_refit=n_refit, return_counts=True)


def _assert_exact(got, want, what):
    for key in ("hyp_count", "best", "n_shared", "n_inliers", "status", "inlier"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")


def _assert_close(got, want, margin, what, exact_fit=False):
    """H, the RMS (relative to its own size; to the coordinates' where every inlier is fitted to rounding) and the ratio of the
    pairs of status 0 within ``margin``; the other pairs NaN, without inliers."""
    ok = want["status"] == 0
    bad = ~ok
    assert np.isnan(got["H"][bad]).all() and np.isnan(got["quality"][bad]).all()
    assert not got["inlier"][bad].any() and not got["n_inliers"][bad].any()
    if not ok.any():
        return
    d = np.abs(got["H"][ok] - want["H"][ok]).max()
    dq = (np.abs(got["quality"][ok, 0] - want["quality"][ok, 0]) / (1.0 if exact_fit else want["quality"][ok, 0])).max()
    dr = np.abs(got["quality"][ok, 1] - want["quality"][ok, 1]).max()
    print(f"{what}: max |dH| {d:.3e}, RMS relative {dq:.3e}, ratio {dr:.3e} (margin {margin:.1e})")
    assert d <= margin and dq <= margin and dr <= margin
    Hm = got["H"][ok].reshape(-1, 9)
    np.testing.assert_allclose(np.linalg.norm(Hm, axis=1), 1.0, rtol=0, atol=1e-14)
    assert (Hm[np.arange(len(Hm)), np.abs(Hm).argmax(axis=1)] > 0).all()


def _assert_same_rows(a, rows_a, b, rows_b, what):
    for key in KEYS:
        x, y = np.ascontiguousarray(a[key][rows_a]), np.ascontiguousarray(b[key][rows_b])
        assert x.tobytes() == y.tobytes(), f"{what}: {key}"


@pytest.mark.parametrize("name", sorted(HC.PARITY))
def test_parity_with_the_reference(name):
    """80 x 3 (one chunk), 257 x 2 (two chunks, the last of one point), pixel units; every pair and one reversed; two calls bitwise."""
    pt_ptr, cam, xy, m, pairs, thr, H, seed, bad, _ = HC.case(name)
    got, want = _run(pt_ptr, cam, xy, m, pairs, thr, H, seed), HC.reference(name)
    _assert_exact(got, want, name)
    _assert_close(got, want, HC.MARGIN * HC.HOST_DIFF[name], name)
    again = _run(pt_ptr, cam, xy, m, pairs, thr, H, seed)
    _assert_same_rows(got, slice(None), again, slice(None), f"{name}: two calls")
    zero = _run(pt_ptr, cam, xy, m, pairs, thr, H, seed, 0)
    _assert_exact(zero, HC.reference(name, "closed", 0), name + ", n_refit = 0")
    np.testing.assert_array_equal(zero["n_inliers"], want["hyp_count"].max(axis=1))


def test_a_reversed_pair_gives_the_inverse_relation():
    """The noise-free plane, (k, l) and (l, k): every hypothesis is the exact homography, all 80 points are inliers, and the two
    matrices are inverses of each other."""
    pt_ptr, cam, xy, m, pairs = HC.noise_free_case()
    got = _run(pt_ptr, cam, xy, m, pairs, HC.THRESHOLD, 16, 1)
    want = HR.homography_robust(pt_ptr, cam, xy, m, pairs, HC.THRESHOLD, 16, 1, 2)
    _assert_exact(got, want, "noise_free")
    margin = HC.MARGIN * HC.HOST_DIFF["noise_free"]
    _assert_close(got, want, margin, "noise_free", exact_fit=True)
    assert (got["hyp_count"] == 80).all() and got["n_inliers"].tolist() == [80, 80]
    d = np.abs(HR.unit(np.linalg.inv(got["H"][0])) - got["H"][1]).max()
    print(f"|unit(inv(H_kl)) - H_lk| = {d:.3e} (margin {margin:.1e})")
    assert d <= margin


def test_statuses_side_by_side_and_the_minimum_point_counts():
    """Status 0, 1 (three shared points) and 2 (a collinear image) in one call; exactly four shared points: every hypothesis is the
    same sample and the status is 0; three: status 1; status 4 from data at one hypothesis."""
    ptr, cam, xy, m, pairs, want_st = HC.mixed_case()
    got, want = _run(ptr, cam, xy, m, pairs, HC.THRESHOLD, 64, 2), HC.mixed_reference()
    _assert_exact(got, want, "mixed")
    _assert_close(got, want, HC.MARGIN * HC.HOST_DIFF["mixed"], "mixed")
    np.testing.assert_array_equal(got["status"], want_st)
    assert (got["best"][want_st != 0] == -1).all() and (got["hyp_count"][want_st != 0] == -1).all()
    alone = _run(ptr, cam, xy, m, pairs[want_st == 0], HC.THRESHOLD, 64, 2)
    _assert_same_rows(got, want_st == 0, alone, slice(None), "the status-0 pairs among the others and alone")
    pt_ptr, cam, xy, m, pairs = HC.few_case(4)
    got, want = _run(pt_ptr, cam, xy, m, pairs, HC.THRESHOLD, 64, 2), HR.homography_robust(pt_ptr, cam, xy, m, pairs, HC.THRESHOLD, 64, 2, 2)
    _assert_exact(got, want, "four")
    _assert_close(got, want, HC.MARGIN * HC.HOST_DIFF["four"], "four", exact_fit=True)
    assert got["status"].tolist() == [0] and (got["hyp_count"] == 4).all() and got["n_shared"][0] == 4
    pt_ptr, cam, xy, m, pairs = HC.few_case(3)
    got = _run(pt_ptr, cam, xy, m, pairs, HC.THRESHOLD, 64, 2)
    assert got["status"].tolist() == [1] and got["n_shared"][0] == 3 and (got["hyp_count"] == -1).all() and np.isnan(got["H"]).all()


@pytest.mark.parametrize("H", [1, 64, 65])
def test_hypothesis_block_boundaries(H):
    """One hypothesis (status 4 where it counts fewer than four points), a full LDS block, and a second block of one."""
    pt_ptr, cam, xy, m, pairs, thr, _, seed, _, _ = HC.case("planar80x3")
    got, want = _run(pt_ptr, cam, xy, m, pairs, thr, H, seed), HC.reference("planar80x3", n_hyp=H)
    _assert_exact(got, want, f"H = {H}")
    _assert_close(got, want, HC.MARGIN * HC.HOST_DIFF[f"h{H}"], f"H = {H}")
    assert got["hyp_count"].shape == (len(pairs), H)
    if H == 1:
        assert got["status"].tolist() == [0, 0, 4, 4] and (got["best"] == 0).all() and (got["hyp_count"][2:, 0] < 4).all()


@pytest.mark.parametrize("which", ["four", "eighty"])
def test_maximum_hypothesis_count(which):
    """n_hypotheses = 65 536 on the 4-point and the 80-point pair: 1024 hypothesis blocks; the sampled entries of the table."""
    if which == "four":
        pt_ptr, cam, xy, m, pairs = HC.few_case(4)
        thr, seed = HC.THRESHOLD, 2
    else:
        pt_ptr, cam, xy, m, pairs, thr, _, seed, _, _ = HC.case("planar80x3")
        pairs = pairs[2:3]
    got = _run(pt_ptr, cam, xy, m, pairs, thr, HC.MAX_HYP, seed)
    hc = got["hyp_count"][0]
    hs, counts, _, _ = HC.max_hyp_reference(which)
    np.testing.assert_array_equal(hc[hs], counts)
    assert hc.shape == (HC.MAX_HYP,) and got["status"][0] == 0 and got["best"][0] == np.argmax(hc)
    if which == "four":
        assert (hc == 4).all()
    else:
        low = _run(pt_ptr, cam, xy, m, pairs, thr, 512, seed)
        assert hc[:512].tobytes() == low["hyp_count"][0].tobytes()  # a hypothesis depends on (seed, k, l, h) only
    print(f"H = 65536, {which}: best {got['best'][0]} with count {hc.max()}, {len(hs)} counts compared with the reference")


def test_refit_counts_with_pairs_leaving_at_different_refits():
    pt_ptr, cam, xy, m, pairs, _, H, seed, _, _ = HC.case("planar80x3")
    for r in HC.REFIT_COUNTS:
        got, want = _run(pt_ptr, cam, xy, m, pairs, HC.REFIT_THRESHOLD, H, seed, r), HC.refit_reference(r)
        _assert_exact(got, want, f"n_refit = {r}")
        _assert_close(got, want, HC.MARGIN * HC.HOST_DIFF["refits"], f"n_refit = {r}")
    assert len(set(RC.end_refit(want, 16).tolist())) >= 2
    for p in range(len(pairs)):
        one = _run(pt_ptr, cam, xy, m, pairs[p:p + 1], HC.REFIT_THRESHOLD, H, seed, 16)
        _assert_same_rows(got, slice(p, p + 1), one, slice(None), f"pair {pairs[p].tolist()} in the call and alone")


def test_pairs_cycled_past_one_tile():
    """14 pairs at 65 536 hypotheses: tiles of 12 (the bytes of H and H^-1 per hypothesis), mixed statuses in both tiles; every pair
    is bitwise the pair of the 9-pair call, which is one tile."""
    ptr, cam, xy, m, pairs, want_st = HC.mixed_case()
    n = len(ptr) - 1
    assert HC.pair_tile(n, 14, HC.MAX_HYP) == 12 and HC.pair_tile(n, 9, HC.MAX_HYP) == 9
    many = HC.C.cycled(pairs, 14)
    got, base = _run(ptr, cam, xy, m, many, HC.THRESHOLD, HC.MAX_HYP, 2), _run(ptr, cam, xy, m, pairs, HC.THRESHOLD, HC.MAX_HYP, 2)
    idx = np.arange(14) % 9
    np.testing.assert_array_equal(got["status"], want_st[idx])
    _assert_same_rows(got, slice(None), base, idx, "cycled")
    np.testing.assert_array_equal(base["hyp_count"][:, :64], HC.mixed_reference()["hyp_count"])


def test_relative_pose_from_the_homography():
    """The contaminated planar pair (1, 2): model="homography" and "auto" give the reference's pose."""
    pt_ptr, cam, xy, m, _, thr, H, seed, _, K = HC.case("planar80x3")
    Rr, tr, Xr, ir = HC.reference_pose()
    margin = HC.MARGIN * HC.POSE_HOST_DIFF
    for model in ("homography", "auto"):
        R, t, X, info = relative_pose(pt_ptr, cam, xy, K, (1, 2), ransac_threshold=thr, n_hypotheses=H, seed=seed, model=model)
        d = max(np.abs(R - Rr).max(), np.abs(t - tr).max())
        print(f"model = {model}: |d(R, t)| to the reference {d:.3e} (margin {margin:.1e}), n_front {info['n_front']}, rms {info['rms']}")
        assert info["status"] == 0 and info["model"] == "homography" and info["ambiguous"] == ir["ambiguous"] is False
        np.testing.assert_array_equal(info["n_front"], ir["n_front"])
        np.testing.assert_array_equal(info["inlier"], ir["inlier"])
        assert d <= margin and info["n_inliers_H"] == 56 and len(info["candidates"]) == 4
        ok = np.isfinite(Xr).all(axis=1)
        np.testing.assert_array_equal(np.isfinite(X).all(axis=1), ok)
        assert np.abs(info["plane"][0] - ir["plane"][0]).max() <= margin and abs(info["plane"][1] - ir["plane"][1]) <= margin
    e = HC.pose_error(R, t, *HC.true_pose("planar80x3", 1, 2))
    assert e <= HC.POSE_H_ERR * 1.01
    with pytest.raises(ValueError, match="needs ransac_threshold"):
        relative_pose(pt_ptr, cam, xy, K, (1, 2), model="auto", homography_threshold=thr)
    with pytest.raises(ValueError, match="model = 'plane'"):
        relative_pose(pt_ptr, cam, xy, K, (1, 2), model="plane")
    # a general scene: "auto" is the fundamental route, bit for bit
    pt_ptr, cam, xy, m, _, thr, H, seed, _ = RC.case("300x8")
    K = np.tile(np.eye(3), (m, 1, 1))
    a = relative_pose(pt_ptr, cam, xy, K, (0, 1), ransac_threshold=thr, n_hypotheses=H, seed=seed, model="auto")
    b = relative_pose(pt_ptr, cam, xy, K, (0, 1), ransac_threshold=thr, n_hypotheses=H, seed=seed)
    assert a[3]["model"] == b[3]["model"] == "fundamental" and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    ratio = a[3]["n_inliers_H"] / a[3]["n_inliers_F"]
    assert abs(ratio - HC.RATIO_GENERAL["300x8"]) <= 5e-4


def _robust_cost(n, pt_ptr, cam, xy, X, K, R, t, delta):
    eng = _mvba.HipEngine(n, 8, pt_ptr, cam, xy, 1.0, "x-up_z-forward", loss="huber", loss_scale=delta)
    eng.set_params(X, K[:, 0, 0], K[:, :2, 2], t, R)
    E = eng.cost()
    eng.close()
    return E


def test_bootstrap_of_a_planar_scene_then_robust_bundle_adjustment():
    """The planar 300 x 8 twin, 20 % of the observations of cameras 2 .. 7 replaced: model="auto" starts from the homography,
    registers every camera the reference registers, in its order, from clean observations only, and Huber BA from there ends
    below the cost of the ground truth."""
    sc, Xp, xy, replaced = HC.bootstrap_case()
    K, R, t, X, info = bootstrap(sc.pt_ptr, sc.cam_idx, xy, sc.init_K, start_pair=(0, 1), max_rms=0.01, ransac_threshold=HC.THRESHOLD,
                                 pose_threshold=HC.THRESHOLD, seed=1, model="auto")
    Rr, tr, Xr, ir = HC.reference_bootstrap()
    print(f"planar bootstrap: model {info['model']}, order {info['order']} (reference {ir['order']}), {info['point_ok'].sum()} points")
    assert info["model"] == "homography" and info["order"] == ir["order"] and info["camera_ok"].all()
    np.testing.assert_array_equal(info["camera_ok"], ir["camera_ok"])
    assert not (info["inlier"] & replaced).any()
    ok = info["point_ok"]
    ptr, cam, z, pid, _ = restrict_observations(sc.pt_ptr, sc.cam_idx, xy, ok, info["camera_ok"])
    delta = 5e-3
    ba = BundleAdjuster.from_observations(len(pid), 8, ptr, cam, z, X[pid], K, R, t, axis=info["axis"], loss="huber", loss_scale=delta)
    E0 = ba._engine.cost()
    ba.optimize()
    E, E_gt = ba._engine.cost(), _robust_cost(len(pid), ptr, cam, z, Xp[pid], sc.K_gt, sc.R_gt, sc.t_gt, delta)
    print(f"huber cost {E0:.4e} -> {E:.4e}, ground truth {E_gt:.4e}")
    assert E < E_gt


def test_bootstrap_from_an_ambiguous_start():
    """Two candidates put every inlier of the start pair in front: relative_pose says so, bootstrap runs its first registration
    round under both and ends where the reference ends."""
    from lib.initialization import engine_intrinsics

    sc, ptr, cam, xy, replaced, _ = HC.ambiguous_case()
    Kxy = engine_intrinsics(sc.init_K)
    ir = HR.homography_pose(ptr, cam, xy, Kxy, (0, 1), HC.THRESHOLD, 512, 1)[3]
    R2, t2, X2, info = relative_pose(ptr, cam, xy, Kxy, (0, 1), ransac_threshold=HC.THRESHOLD, seed=1, model="homography")
    assert info["ambiguous"] and ir["ambiguous"] and info["best_candidate"] == ir["best_candidate"]
    np.testing.assert_array_equal(info["n_front"], ir["n_front"])
    other = [c for c in range(4) if c != info["best_candidate"] and info["n_front"][c] == info["n_front"].max()][0]
    Ro, to, Xo, io = relative_pose(ptr, cam, xy, Kxy, (0, 1), ransac_threshold=HC.THRESHOLD, seed=1, model="homography", _candidate=other)
    assert io["status"] == 0 and io["best_candidate"] == other and np.abs(Ro[1] - R2[1]).max() > 0.1
    assert np.isfinite(Xo).all(axis=1).sum() == np.isfinite(X2).all(axis=1).sum() == 33
    K, R, t, X, bi = bootstrap(ptr, cam, xy, sc.init_K, start_pair=(0, 1), max_rms=0.01, ransac_threshold=HC.THRESHOLD,
                               pose_threshold=HC.THRESHOLD, seed=1, model="auto")
    Rr, tr, Xr, br = HC.ambiguous_reference()
    d = max(np.abs(R[:2] - Rr[:2]).max(), np.abs(t[:2] - tr[:2]).max())
    print(f"ambiguous start: order {bi['order']} (reference {br['order']}), |d(R, t)| of the pair to the reference {d:.3e}")
    assert bi["model"] == "homography" and bi["order"] == br["order"] and bi["camera_ok"].all() and not (bi["inlier"] & replaced).any()
    assert d <= HC.MARGIN * HC.POSE_HOST_DIFF
    with pytest.raises(ValueError, match="_candidate = 7"):
        relative_pose(ptr, cam, xy, Kxy, (0, 1), ransac_threshold=HC.THRESHOLD, seed=1, model="homography", _candidate=7)
    # the other two forms of the first registration round run from the same start (contaminated cameras: what they register is
    # not the subject here, that the round under both candidates runs and the start stays the homography's is)
    for kw in ({"resect_threshold": HC.THRESHOLD}, {}):
        bo = bootstrap(ptr, cam, xy, sc.init_K, start_pair=(0, 1), max_rms=0.01, ransac_threshold=HC.THRESHOLD, seed=1, model="homography", **kw)[4]
        assert bo["model"] == "homography" and bo["order"][:2] == [0, 1] and bo["camera_ok"][:2].all()


def test_fundamental_matrix_through_the_shared_loop():
    """robust_fundamental_matrices on "300x8" against tests/_ransac_ref.py: the F fit of the loop the two models share."""
    pt_ptr, cam, xy, m, pairs, thr, H, seed, _ = RC.case("300x8")
    F, info = robust_fundamental_matrices(pt_ptr, cam, xy, m, pairs, thr, n_hypotheses=H, seed=seed)
    want = RC.reference("300x8")
    for key in ("best", "n_shared", "n_inliers", "status", "inlier"):
        np.testing.assert_array_equal(info[key], want[key], err_msg=key)
    margin = RC.MARGIN * RC.RANSAC_HOST_DIFF["300x8"]
    d = np.abs(F - want["F"]).max()
    dq = (np.abs(info["quality"][:, 0] - want["quality"][:, 0]) / want["quality"][:, 0]).max()
    print(f"F through robust_pairs: max |dF| {d:.3e}, Sampson RMS relative {dq:.3e} (margin {margin:.1e})")
    assert d <= margin and dq <= margin and np.abs(info["quality"][:, 1] - want["quality"][:, 1]).max() <= margin
    Hm, hi = robust_homographies(pt_ptr, cam, xy, m, pairs[:1], thr, n_hypotheses=H, seed=seed)
    assert hi["status"][0] == 0 and 0.0 < hi["confidence"][0] <= 1.0 and set(hi["timings_ms"]) == {"upload", "score", "refit", "other"}
