"""Robust two-view geometry on the device: mvba_two_view_robust against the NumPy restatement of
tests/_ransac_ref.py -- count tables, best hypotheses, inlier masks and statuses EXACTLY (tests/test_ransac_cpu.py asserts the
premises under which that may be asked), F and the Sampson RMS within 100 x the host-versus-host difference of the very case
(tests/_ransac_cases.py) --, and relative_pose and bootstrap with ``ransac_threshold`` on contaminated tracks."""
import numpy as np
import pytest

import _ransac_cases as RC
import _twoview_cases as C
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster
from lib.initialization import bootstrap, relative_pose, restrict_observations, robust_fundamental_matrices

pytestmark = pytest.mark.gpu

KEYS = ("F", "quality", "n_shared", "n_inliers", "best", "status", "inlier", "hyp_count")


def _run(pt_ptr, cam, xy, m, pairs, thr, H, seed, n_refit=2):
    return _mvba.two_view_robust(pt_ptr, cam, xy, m, pairs, thr, n_hypotheses=H, seed=seed, n_refit=n_refit, return_counts=True)


def _assert_exact(got, want, what):
    for key in ("hyp_count", "best", "n_shared", "n_inliers", "status", "inlier"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")


def _assert_close(got, want, margin, scale_xy, what):
    ok = want["status"] == 0
    bad = ~ok
    assert np.isnan(got["F"][bad]).all() and np.isnan(got["quality"][bad]).all()
    d = np.abs(got["F"][ok] - want["F"][ok]).max()
    scale = np.where(want["n_inliers"][ok] > 8, want["quality"][ok, 0], scale_xy)
    dq = (np.abs(got["quality"][ok, 0] - want["quality"][ok, 0]) / scale).max()
    dr = np.abs(got["quality"][ok, 1] - want["quality"][ok, 1]).max()
    print(f"{what}: max |dF| {d:.3e}, Sampson RMS relative {dq:.3e}, ratio {dr:.3e} (margin {margin:.1e})")
    assert d <= margin and dq <= margin and dr <= margin


@pytest.mark.parametrize("name", sorted(RC.PARITY))
def test_parity(name):
    pt_ptr, cam, xy, m, pairs, thr, H, seed, _ = RC.case(name)
    got, want = _run(pt_ptr, cam, xy, m, pairs, thr, H, seed), RC.reference(name)
    _assert_exact(got, want, name)
    assert (want["status"] == 0).all()
    _assert_close(got, want, RC.MARGIN * RC.RANSAC_HOST_DIFF[name], np.abs(xy).max(), name)
    assert set(got["timings_ms"]) == {"upload", "score", "refit", "other"} and got["timings_ms"]["score"] > 0
    if name == "300x8":  # the public call; and without refits: the best hypothesis itself, made rank 2 on the host
        F2, info = robust_fundamental_matrices(pt_ptr, cam, xy, m, pairs, thr, n_hypotheses=H, seed=seed)
        assert F2.tobytes() == got["F"].tobytes() and np.array_equal(info["inlier"], got["inlier"])
        w = want["n_inliers"] / want["n_shared"]
        np.testing.assert_allclose(info["confidence"], 1.0 - (1.0 - w ** 8) ** H, rtol=1e-12)
        got0, want0 = _run(pt_ptr, cam, xy, m, pairs, thr, H, seed, n_refit=0), RC.reference(name, "eigh", 0)
        _assert_exact(got0, want0, name + ", n_refit = 0")
        np.testing.assert_array_equal(got0["n_inliers"], want0["hyp_count"].max(axis=1))
        # the hypothesis's own conditioning (lambda_2 / lambda_max down to 1e-9 here) enters F: the host-vs-host figure of this route
        ref_svd = RC.reference(name, "svd", 0)
        margin0 = RC.MARGIN * max(np.abs(want0["F"] - ref_svd["F"]).max(), RC.RANSAC_HOST_DIFF[name])
        _assert_close(got0, want0, margin0, np.abs(xy).max(), name + ", n_refit = 0")
        assert (got0["quality"][:, 1] == 0).all()
    if name == "257x2":  # the list form and the dense grid are one computation
        dense = _run(None, None, xy.reshape(257, 2, 2), 2, pairs, thr, H, seed)
        for key in KEYS:
            assert dense[key].tobytes() == got[key].tobytes(), key


def test_status_cases():
    for name, (pt_ptr, cam, xy, m, pairs, want_status) in RC.status_cases().items():
        got = _run(pt_ptr, cam, xy, m, pairs, RC.THRESHOLD, 16, 1)
        want = RC.RR.two_view_robust(pt_ptr, cam, xy, m, pairs, RC.THRESHOLD, 16, 1, 2)
        _assert_exact(got, want, name)
        assert got["status"].tolist() == [want_status], name
        hc = got["hyp_count"][0]
        if name == "eight":  # the premise: exactly 8 shared points, every hypothesis is the same set; the rejection loop ends
            assert got["n_shared"][0] == 8 and (hc == 8).all() and got["best"][0] == 0 and got["n_inliers"][0] == 8
            assert np.isfinite(got["F"]).all() and got["inlier"][0].sum() == 8
        elif name == "seven":
            assert got["n_shared"][0] == 7 and (hc == -1).all() and got["best"][0] == -1
        elif name == "planar":  # noise-free points in a plane: every minimal sample has a null space of dimension 3
            assert got["n_shared"][0] == 80 and (hc == -1).all()
        else:  # every image-l observation replaced: no geometry, but a hypothesis still counts its own sample
            assert got["n_shared"][0] == 80 and (hc >= 8).all() and got["n_inliers"][0] < 40
        if want_status:
            assert np.isnan(got["F"]).all() and np.isnan(got["quality"]).all() and not got["inlier"].any() and got["n_inliers"][0] == 0


def test_pair_tiles_under_the_byte_bound():
    """170 pairs on 16 641 points at 8 hypotheses: 128 MiB / (48 x 16641 + 160 x 8) = 167 pairs per tile, so the call takes
    two; every occurrence of a pair is bitwise its first, and the first six are the call with six pairs."""
    pt_ptr, cam, xy, m, six = C.case("16641x3")
    n_pairs, H = 170, 8
    assert RC.pair_tile(len(pt_ptr) - 1, n_pairs, H) == 167 < n_pairs
    out = _run(pt_ptr, cam, xy, m, C.cycled(six, n_pairs), RC.THRESHOLD, H, 1)
    one = _run(pt_ptr, cam, xy, m, six, RC.THRESHOLD, H, 1)
    assert (out["status"] == 0).all() and (out["n_shared"] == 16641).all()
    for key in KEYS:
        a = np.ascontiguousarray(out[key]).reshape(n_pairs, -1)
        first = a[np.arange(n_pairs) % 6]
        assert a.tobytes() == first.tobytes(), key
        assert a[:6].tobytes() == np.ascontiguousarray(one[key]).reshape(6, -1).tobytes(), key


def test_bad_arguments():
    pt_ptr, cam, xy, m, _ = C.case("300x8")
    for kw, text in (({"threshold": 0.0}, "threshold = 0.0"), ({"threshold": np.inf}, "threshold = inf"), ({"n_hypotheses": 0}, "n_hypotheses = 0"),
                     ({"n_hypotheses": 65537}, "n_hypotheses = 65537"), ({"n_refit": -1}, "n_refit = -1"), ({"n_refit": 17}, "n_refit = 17")):
        args = {"threshold": 0.01, **kw}
        with pytest.raises(ValueError, match=text):
            _mvba.two_view_robust(pt_ptr, cam, xy, m, [(0, 1)], **args)
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        _mvba.two_view_robust(pt_ptr, cam, xy, m, [(0, 1), (4, 4)], 0.01)
    bad = cam.copy()
    bad[[0, 1]] = bad[[1, 0]]
    with pytest.raises(ValueError, match="not ascending within point 0"):
        _mvba.two_view_robust(pt_ptr, bad, xy, m, [(0, 1)], 0.01)
    out = _mvba.two_view_robust(pt_ptr, cam, xy, m, np.zeros((0, 2), np.int32), 0.01)
    assert out["F"].shape == (0, 3, 3) and out["inlier"].shape == (0, 300)


def test_two_calls_are_bitwise_equal_and_the_seed_moves_only_the_sample():
    for name in ("300x8", "2000x3"):
        pt_ptr, cam, xy, m, pairs, thr, H, seed, _ = RC.case(name)
        a, b = _run(pt_ptr, cam, xy, m, pairs, thr, H, seed), _run(pt_ptr, cam, xy, m, pairs, thr, H, seed)
        for key in KEYS:
            assert a[key].tobytes() == b[key].tobytes(), (name, key)
        one = _run(pt_ptr, cam, xy, m, pairs[1:2], thr, H, seed)  # a pair's result does not depend on the other pairs of the call
        for key in KEYS:
            assert one[key].tobytes() == a[key][1:2].tobytes(), (name, key)
    pt_ptr, cam, xy, m, pairs, thr, H, seed, bad = RC.case("300x8")
    a, c = _run(pt_ptr, cam, xy, m, pairs[:1], thr, H, seed), _run(pt_ptr, cam, xy, m, pairs[:1], thr, H, seed + 1)
    assert a["best"][0] != c["best"][0] and not np.array_equal(a["hyp_count"], c["hyp_count"])
    np.testing.assert_array_equal(a["inlier"], c["inlier"])


def test_relative_pose_on_a_contaminated_pair():
    sc, xy, bad = RC.pose_case()
    R, t, X, info = relative_pose(sc.pt_ptr, sc.cam_idx, xy, sc.K_gt, (0, 1), ransac_threshold=RC.THRESHOLD, seed=1)
    Rr, tr, Xr, ir = RC.reference_pose()
    d = max(np.abs(R - Rr).max(), np.abs(t - tr).max())
    e = RC.pose_error(sc, R, t)
    print(f"robust pose: |d| to the reference {d:.2e} (margin {RC.MARGIN * RC.POSE_HOST_DIFF:.1e}), error {e:.2e} "
          f"(bound {RC.POSE_FACTOR} x {RC.POSE_CLEAN_ERR:.1e})")
    assert info["status"] == 0 and info["n_inliers"] == 56 == ir["n_inliers"] and info["n_shared"] == 80
    np.testing.assert_array_equal(info["inlier"], ir["inlier"])
    # (which of the four candidates wins is not compared: E has two equal singular values, so its SVD -- and with it the order
    # of the candidates -- turns on the last bit of F; the existing two-view pose test compares the sorted counts as well)
    assert sorted(info["n_front"]) == sorted(ir["n_front"]) == [0, 0, 0, 56]
    np.testing.assert_array_equal(np.isfinite(X).all(axis=1), info["inlier"])  # the other shared points stay NaN
    assert d <= RC.MARGIN * RC.POSE_HOST_DIFF
    assert e <= RC.POSE_FACTOR * RC.POSE_CLEAN_ERR
    np.testing.assert_allclose(X[info["inlier"]], Xr[info["inlier"]], rtol=0, atol=1e-10)


def _robust_cost(n, pt_ptr, cam, xy, X, K, R, t, delta):
    eng = _mvba.HipEngine(n, 8, pt_ptr, cam, xy, 1.0, "x-up_z-forward", loss="huber", loss_scale=delta)
    eng.set_params(X, K[:, 0, 0], K[:, :2, 2], t, R)
    E = eng.cost()
    eng.close()
    return E


def test_bootstrap_on_contaminated_tracks_then_robust_bundle_adjustment():
    sc, xy, replaced = RC.bootstrap_case()
    K, R, t, X, info = bootstrap(sc.pt_ptr, sc.cam_idx, xy, sc.init_K, start_pair=(0, 1), ransac_threshold=RC.THRESHOLD, max_rms=0.01, seed=1)
    Rr, tr, Xr, ir = RC.reference_bootstrap()
    np.testing.assert_array_equal(info["camera_ok"], ir["camera_ok"])
    np.testing.assert_array_equal(info["point_ok"], ir["point_ok"])
    assert info["order"] == ir["order"] and info["camera_ok"].all()
    ok = info["point_ok"]
    d = max(np.abs(R - Rr).max(), np.abs(t - tr).max(), np.abs(X[ok] - Xr[ok]).max())
    print(f"bootstrap: {ok.sum()} points, |d| to the reference {d:.2e} (margin {RC.MARGIN * RC.BOOT_HOST_DIFF:.1e})")
    assert d <= RC.MARGIN * RC.BOOT_HOST_DIFF
    ptr, cam, z, pid, _ = restrict_observations(sc.pt_ptr, sc.cam_idx, xy, ok, info["camera_ok"])
    delta = 5e-3  # five times the noise: the replaced observations are far beyond it
    ba = BundleAdjuster.from_observations(len(pid), 8, ptr, cam, z, X[pid], K, R, t, axis=info["axis"], loss="huber", loss_scale=delta)
    E0 = ba._engine.cost()
    ba.optimize()
    E, E_gt = ba._engine.cost(), _robust_cost(len(pid), ptr, cam, z, sc.X_gt[pid], sc.K_gt, sc.R_gt, sc.t_gt, delta)
    print(f"huber cost {E0:.4e} -> {E:.4e}, ground truth {E_gt:.4e}")
    assert E < E_gt
