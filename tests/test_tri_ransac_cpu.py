"""Robust triangulation, the part that needs no GPU: the hypothesis rule libmvba.so exports is the reference's,
the premises under which the GPU parity tests may ask for EXACT count tables hold on every case, the reference recovers the
clean observations of every point that has three, and the host-versus-host differences that set the GPU margins are what
tests/_tri_ransac_cases.py records."""
import ctypes
import os

import numpy as np
import pytest

import _tri_ransac_cases as TC
import _tri_ransac_ref as TR
from lib import _mvba
from lib.initialization import ransac_sample, triangulate_sample

EXACT = ("hyp_count", "status", "best", "n_inliers", "inlier", "sizes", "end")

# (seed, point, h, deg, n_hypotheses): one pair; three observations; 28 pairs in 64 (the last pair, the first entry past them);
# exactly as many pairs as hypotheses; one more pair than hypotheses (sampled); degree 70; the largest degree, seed and table
SAMPLE_TABLE = [(0, 0, 0, 2, 1), (1, 5, 2, 3, 64), (1, 299, 27, 8, 64), (1, 299, 28, 8, 64), (7, 3, 44, 10, 45), (7, 3, 43, 10, 44),
                (1, 64, 63, 70, 64), (1, 64, 16, 70, 17), ((1 << 64) - 1, (1 << 31) - 1, 4095, (1 << 31) - 1, 4096), (3, 9, 4094, 91, 4096)]


@pytest.mark.parametrize("seed,a,h,deg,H", SAMPLE_TABLE)
def test_exported_hypothesis_rule_is_the_reference(seed, a, h, deg, H):
    got, want = triangulate_sample(seed, a, h, deg, H), TR.sample(seed, a, h, deg, H)
    assert got.dtype == np.int64 and tuple(got.tolist()) == want
    n_pairs = deg * (deg - 1) // 2
    if n_pairs <= H:  # exhaustive: the table lists every pair once, in lexicographic order, then -1
        table = [tuple(triangulate_sample(seed, a, g, deg, H).tolist()) for g in range(H)]
        assert table[:n_pairs] == [(i, j) for i in range(deg) for j in range(i + 1, deg)] and set(table[n_pairs:]) <= {(-1, -1)}
    else:  # sampled: the first two draws of the generator the other two RANSACs use, sorted
        assert 0 <= got[0] < got[1] < deg
        if deg >= 8:
            assert got.tolist() == sorted(ransac_sample(seed, a, a, h, deg)[:2].tolist())


def test_sample_depends_on_point_and_seed_and_rejects_bad_arguments():
    assert not np.array_equal([triangulate_sample(1, 0, h, 70, 64) for h in range(8)], [triangulate_sample(1, 1, h, 70, 64) for h in range(8)])
    assert not np.array_equal([triangulate_sample(1, 0, h, 70, 64) for h in range(8)], [triangulate_sample(2, 0, h, 70, 64) for h in range(8)])
    for args, text in (((0, 0, 0, 1, 64), "deg = 1"), ((0, 0, 0, 1 << 31, 64), "deg = 2147483648"), ((0, 0, -1, 8, 64), "h = -1"),
                       ((0, -2, 0, 8, 64), "point = -2"), ((0, 0, 64, 8, 64), "h = 64"), ((0, 0, 0, 8, 0), "n_hypotheses = 0"),
                       ((0, 0, 0, 8, 4097), "n_hypotheses = 4097")):
        with pytest.raises(ValueError, match=text):
            triangulate_sample(*args)


def test_library_exports_the_entry_points_and_checks_arguments_without_a_device():
    assert "mvba_triangulate_robust" in _mvba.SIGNATURES and "mvba_triangulate_sample" in _mvba.SIGNATURES
    lib = ctypes.CDLL(_mvba.LIB_PATH)
    for name in ("mvba_triangulate_robust", "mvba_triangulate_sample"):
        assert hasattr(lib, name), name
    lib = _mvba.load_library()
    i32, i64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    K, R, t, pt_ptr, cam, xy, thr, _, _ = TC.case("300x8")
    K, R, t, xy, X = (np.ascontiguousarray(v) for v in (K, R, t, xy, np.empty((300, 3))))

    def call(thr=thr, H=16, n_refine=2, n_refit=2, X=X, m=8):
        rc = lib.mvba_triangulate_robust(_mvba._ptr(K), _mvba._ptr(R), _mvba._ptr(t), m, 300, pt_ptr.ctypes.data_as(i64), cam.ctypes.data_as(i32),
                                         _mvba._ptr(xy), len(cam), thr, H, 1, n_refine, n_refit, None if X is None else _mvba._ptr(X), None, None,
                                         None, None, None, None, None, -1)
        return rc, lib.mvba_last_error().decode()

    for kw, text in (({"thr": 0.0}, "threshold = 0.0"), ({"thr": float("nan")}, "threshold = nan"), ({"thr": -0.5}, "threshold = -0.5"),
                     ({"H": 0}, "n_hypotheses = 0"), ({"H": 4097}, "n_hypotheses = 4097"), ({"n_refit": -1}, "n_refit = -1"),
                     ({"n_refit": 17}, "n_refit = 17"), ({"n_refine": -1}, "n_refine = -1"), ({"X": None}, "null argument: X"),
                     ({"m": 7}, "cam_idx out of range"), ({"m": 1705}, "too many cameras")):
        rc, msg = call(**kw)
        assert rc == _mvba.MVBA_ERR_BADARG and text in msg, (kw, msg)


def test_triangulate_robust_fails_loudly_without_gpu():
    if os.path.exists(_mvba.LIB_PATH) and _mvba.device_count() > 0:
        pytest.skip("a device is visible")
    K, R, t, pt_ptr, cam, xy, thr, _, _ = TC.case("300x8")
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        _mvba.triangulate_robust(K, R, t, pt_ptr, cam, xy, thr)


def _premises(a, b, what):
    """(a) the two host routes give one count table and everything that follows from it; (b) no distance within 1e-6
    (relative, squared) of the threshold.  (The reference itself asserts (c): where a Gauss-Newton step of the last kept refit
    is a tie, both of its outcomes select the same inliers.)"""
    for key in EXACT:
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what}: {key}")
    margin = min(a["margin"].min(), b["margin"].min())
    print(f"{what}: smallest |d^2 / thr^2 - 1| {margin:.2e}; statuses {np.bincount(a['status'], minlength=5).tolist()}; "
          f"{(a['n_ties'] > 0).sum()} points with a tied Gauss-Newton step")
    assert margin >= 1e-6
    ok = a["status"] == 0
    assert a["alt_X"][ok, 0].tobytes() == a["X"][ok].tobytes() and a["alt_quality"][ok, 0].tobytes() == a["quality"][ok].tobytes()
    bad = a["status"] != 0
    assert np.isnan(a["X"][bad]).all() and np.isnan(a["quality"][bad]).all() and (a["n_inliers"][bad] == 0).all()


def _host_difference(a, b, what, recorded):
    dX, dq = TC.max_diff(a, b)
    d = max(dX, dq.max())
    print(f"{what}: host versus host max |dX| = {dX:.3e}, quality {dq} -> {d:.3e} (recorded {recorded:.1e})")
    assert 0.5 * recorded <= d <= recorded


@pytest.mark.parametrize("name", sorted(TC.PARITY))
def test_parity_premises_and_host_versus_host_difference(name):
    a, b = TC.reference(name), TC.reference(name, 2, 2, "svd", "solve")
    _premises(a, b, name)
    a0, b0 = TC.reference(name, 0, 2), TC.reference(name, 0, 2, "svd", "solve")  # the linear refit: what the margin is measured on
    _premises(a0, b0, name + ", n_refine = 0")
    _host_difference(a0, b0, name + ", n_refine = 0", TC.TRI_RANSAC_HOST_DIFF[name])
    dX, dq = TC.max_diff(a, b)
    assert max(dX, dq.max()) <= TC.TRI_RANSAC_HOST_DIFF[name]  # (refined: the routes agree better, not worse)
    K, _, _, pt_ptr, _, _, _, H, _ = TC.case(name)
    deg = np.full(len(a["X"]), len(K)) if pt_ptr is None else np.diff(pt_ptr)
    exhaustive = deg * (deg - 1) // 2 <= H
    assert ((a["hyp_count"] >= 0).sum(axis=1)[exhaustive] == (deg * (deg - 1) // 2)[exhaustive]).all()
    assert ((a["hyp_count"] >= 0).sum(axis=1)[~exhaustive] == H).all()
    if name.startswith("65x70") or name == "300x1704":
        assert not exhaustive.all()  # the sampled branch
    if name == "300x8":  # without refits X is the best midpoint itself
        m0, n0 = TC.reference(name, 2, 0), TC.reference(name, 2, 0, "svd", "solve")
        _premises(m0, n0, name + ", n_refit = 0")
        _host_difference(m0, n0, name + ", n_refit = 0", TC.MIDPOINT_HOST_DIFF["300x8"])
        ok = m0["status"] == 0
        assert m0["X"][ok].tobytes() == m0["Xmid"][ok].tobytes()
        np.testing.assert_array_equal(m0["n_inliers"][ok], m0["hyp_count"].max(axis=1)[ok])


@pytest.mark.parametrize("name", ["300x8", "pixels", "dense"])
def test_reference_recovers_the_clean_observations(name):
    """20 % of every camera's observations replaced, every pair tried: each point with three or more clean observations gets
    exactly its clean set (225 of 225 on "300x8", where the plain fit of the same lists is off by up to 5e5), and no other
    point gets status 0 unless a replaced observation agrees with two others by chance."""
    ge3, clean = TC.clean_sets(name)
    a = TC.reference(name)
    K, R, t, pt_ptr, cam, xy, thr, H, hit = TC.case(name)
    if pt_ptr is None:
        pt_ptr, _ = TC.IC.ref.dense_list(xy.shape[0], xy.shape[1])
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    assert (a["status"][ge3] == 0).all()
    np.testing.assert_array_equal(a["inlier"][ge3[pt]], clean[ge3[pt]])
    if name == "300x8":
        sc = TC.IC.tri_scene("300x8")
        e = np.linalg.norm(a["X"][ge3] - sc.X_gt[ge3], axis=1)
        plain = TC.IC.ref.triangulate(K, R, t, pt_ptr, cam, xy, 2)[0]
        ep = np.linalg.norm(plain[ge3] - sc.X_gt[ge3], axis=1)
        print(f"{ge3.sum()} points with >= 3 clean observations: robust error max {e.max():.3g} median {np.median(e):.3g}; "
              f"plain fit max {np.nanmax(ep):.3g} median {np.nanmedian(ep):.3g}")
        assert ge3.sum() == 225 and e.max() < 0.03 and np.nanmax(ep) > 1.0


def test_status_shapes_of_the_reference():
    a, b = TC.status_reference(), TC.status_reference("svd", "solve")
    _premises(a, b, "status shapes")
    _host_difference(TC.TR.triangulate_robust(*TC.status_case(), TC.THRESHOLD, TC.STATUS_HYP, TC.SEED, 0, 2),
                     TC.TR.triangulate_robust(*TC.status_case(), TC.THRESHOLD, TC.STATUS_HYP, TC.SEED, 0, 2, "svd", "solve"), "status shapes",
                     TC.STATUS_HOST_DIFF)
    st = a["status"]
    # seen once: 1; two cameras at one centre, and two observations of one direction: parallel rays, every hypothesis degenerate
    assert st[3] == 1 and st[7] == 2 and st[11] == 2
    assert (a["hyp_count"][[3, 7, 11]] == -1).all() and (a["best"][[3, 7, 11]] == -1).all()
    # every observation replaced: no two rays meet; one of three replaced: the clean pair counts 2, below min(deg, 3)
    assert st[TC.ALL_REPLACED] == 4 and st[TC.ONE_OF_THREE] == 4 and a["hyp_count"][TC.ONE_OF_THREE].max() == 2
    assert a["best"][TC.ONE_OF_THREE] == 1  # (the pair (0, 2): the replaced observation is number 1)
    # two observations: one hypothesis, its own two inliers
    assert st[TC.TWO_VIEWS] == 0 and a["n_inliers"][TC.TWO_VIEWS] == 2 and (a["hyp_count"][TC.TWO_VIEWS] == [2] + [-1] * (TC.STATUS_HYP - 1)).all()
    rest = np.setdiff1d(np.arange(40), [3, 7, 11, TC.ALL_REPLACED, TC.ONE_OF_THREE, TC.TWO_VIEWS])
    assert (st[rest] == 0).all() and (a["n_inliers"][rest] == 3).all()


def test_refit_trace_of_the_reference():
    for r in TC.REFIT_COUNTS:
        a, b = TC.refit_reference(r), TC.refit_reference(r, "svd", "solve")
        _premises(a, b, f"refits, n_refit = {r}")
        ok = a["status"] == 0
        assert (a["n_accepted"][ok] == (a["sizes"][ok, 1:] >= 0).sum(axis=1)).all() or r == 0
    a0, a16 = TC.refit_reference(0), TC.refit_reference(16)
    ok = a0["status"] == 0
    assert (a0["n_accepted"] == 0).all() and a0["X"][ok].tobytes() == a0["Xmid"][ok].tobytes()
    _host_difference(a0, TC.refit_reference(0, "svd", "solve"), "refits, n_refit = 0", TC.MIDPOINT_HOST_DIFF["refit"])
    assert (a16["n_accepted"][ok] == 16).all()  # at this threshold no refit shrinks its set: the loop runs to its end
    assert (a16["n_inliers"] != a0["n_inliers"]).any()  # ... and a refit changes a set


def test_bootstrap_reference_on_contaminated_tracks():
    """What the feature buys, on the host: 20 % of the observations of ALL cameras replaced; ransac_threshold and resect_threshold
    set in both runs.  With triangulate_threshold: 8 cameras, 205 points, none triangulated from a replaced observation if it
    has three clean ones, 7 of them farther than 0.1 from the truth (points with fewer than three clean observations, which
    nothing can verify).  Without: all 300 points come back, 88 of them farther than 0.1 from the truth."""
    sc, xy, hit = TC.bootstrap_case()
    Ra, ta, Xa, ia = TC.reference_bootstrap(True)
    Rb, tb, Xb, ib = TC.reference_bootstrap(True, "svd", "solve")
    Rp, tp, Xp, ip = TC.reference_bootstrap(False)
    assert ia["order"] == ib["order"] and len(ia["order"]) == 8 and ia["margin"] >= 1e-6
    for key in ("camera_ok", "point_ok", "obs_ok", "inlier", "tri_inlier"):
        np.testing.assert_array_equal(ia[key], ib[key], err_msg=key)
    ok = ia["point_ok"]
    d = max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max(), np.abs(Xa[ok] - Xb[ok]).max())
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    ge3 = np.bincount(pt[~hit], minlength=sc.n_points) >= 3
    bad_r, bad_p = (TC.point_error(sc, Xa, ok) > TC.BOOT_FAR).sum(), (TC.point_error(sc, Xp, ip["point_ok"]) > TC.BOOT_FAR).sum()
    print(f"robust: {ok.sum()} points, {bad_r} far; plain: {ip['point_ok'].sum()} points, {bad_p} far; host difference {d:.3e} "
          f"(recorded {TC.BOOT_HOST_DIFF:.1e})")
    assert 0.5 * TC.BOOT_HOST_DIFF <= d <= TC.BOOT_HOST_DIFF
    assert not (ia["tri_inlier"] & hit & ge3[pt]).any() and not (ia["tri_inlier"] & ~ia["point_ok"][pt]).any()
    assert (np.bincount(pt[ia["tri_inlier"]], minlength=sc.n_points)[ok] >= 2).all()
    assert ip["camera_ok"].all() and (ok.sum(), bad_r, ip["point_ok"].sum(), bad_p) == TC.BOOT_REFERENCE_FIGURES
    assert bad_p >= TC.BOOT_CONTRAST * max(bad_r, 1)
