"""Robust two-view geometry, the part that needs no GPU: the sample generator libmvba.so exports is the
reference's, the premises under which the GPU parity tests may ask for EXACT count tables hold on every case, the reference
recovers the truth from contaminated pairs, and the host-versus-host differences that set the GPU margins are what
tests/_ransac_cases.py records."""
import ctypes
import os

import numpy as np
import pytest

import _init_cases as IC
import _ransac_cases as RC
import _ransac_ref as RR
import _twoview_cases as C
import _twoview_ref as T
from lib import _mvba
from lib.initialization import ransac_sample

SAMPLE_TABLE = [(0, 0, 1, 0, 8), (1, 0, 1, 5, 80), (1, 0, 1, 511, 80), ((1 << 64) - 1, 3, 2, 7, (1 << 31) - 1), (7, 5, 2, 511, 300),
                (1, 1703, 0, 65535, 9), (12345678901234567890, 6, 7, 3, 8), (1, 1, 0, 5, 80)]


@pytest.mark.parametrize("seed,k,l,h,n", SAMPLE_TABLE)
def test_exported_sample_generator_is_the_reference(seed, k, l, h, n):
    """n = 8 (a permutation), n = 2^31 - 1, k > l, seed = 2^64 - 1: the host instance of the function the kernel runs."""
    got, want = ransac_sample(seed, k, l, h, n), RR.sample(seed, k, l, h, n)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int64 and len(set(got.tolist())) == 8 and (got >= 0).all() and (got < n).all()
    if n == 8:
        assert sorted(got.tolist()) == list(range(8))


def test_sample_depends_on_the_order_of_the_pair_and_rejects_bad_arguments():
    assert not np.array_equal(ransac_sample(1, 0, 1, 5, 80), ransac_sample(1, 1, 0, 5, 80))
    assert not np.array_equal(ransac_sample(1, 0, 1, 5, 80), ransac_sample(2, 0, 1, 5, 80))
    with pytest.raises(ValueError, match="n = 7"):
        ransac_sample(0, 0, 1, 0, 7)
    with pytest.raises(ValueError, match="h = -1"):
        ransac_sample(0, 0, 1, -1, 80)


def test_library_exports_the_robust_entry_points():
    assert "mvba_two_view_robust" in _mvba.SIGNATURES and "mvba_ransac_sample" in _mvba.SIGNATURES
    lib = ctypes.CDLL(_mvba.LIB_PATH)
    for name in ("mvba_two_view_robust", "mvba_ransac_sample"):
        assert hasattr(lib, name), name
    # argument errors come before any device work: they need no GPU
    lib = _mvba.load_library()
    i32, i64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    pt_ptr, cam, xy, m, _ = C.case("300x8")
    F, pairs = np.empty((1, 9)), np.array([(0, 1)], np.int32)

    def call(thr=0.01, H=16, n_refit=2, pair=(0, 1)):
        pairs[0] = pair
        rc = lib.mvba_two_view_robust(300, m, pt_ptr.ctypes.data_as(i64), cam.ctypes.data_as(i32), _mvba._ptr(xy), len(cam), pairs.ctypes.data_as(i32),
                                      1, thr, H, 1, n_refit, _mvba._ptr(F), None, None, None, None, None, None, None, None, -1)
        return rc, lib.mvba_last_error().decode()

    for kw, text in (({"thr": 0.0}, "threshold = 0.0"), ({"thr": float("nan")}, "threshold = nan"), ({"thr": -0.5}, "threshold = -0.5"),
                     ({"H": 0}, "n_hypotheses = 0"), ({"H": 65537}, "n_hypotheses = 65537"), ({"n_refit": -1}, "n_refit = -1"),
                     ({"n_refit": 17}, "n_refit = 17"), ({"pair": (3, 3)}, "(3, 3)"), ({"pair": (2, 8)}, "n_images = 8")):
        rc, msg = call(**kw)
        assert rc == _mvba.MVBA_ERR_BADARG and text in msg, (kw, msg)


def test_two_view_robust_fails_loudly_without_gpu():
    if os.path.exists(_mvba.LIB_PATH) and _mvba.device_count() > 0:
        pytest.skip("a device is visible")
    pt_ptr, cam, xy, m, pairs = C.case("300x8")
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        _mvba.two_view_robust(pt_ptr, cam, xy, m, pairs, 0.01)


def _premises(a, b, what):
    """(a) eigh and SVD null vectors give one count table; (b) no distance within 1e-7 (relative, squared) of the threshold;
    (c) no hypothesis within a factor 100 of the pivot rule; and a hypothesis that is not degenerate counts its own sample."""
    np.testing.assert_array_equal(a["hyp_count"], b["hyp_count"])
    for key in ("status", "best", "n_inliers", "inlier", "n_shared"):
        np.testing.assert_array_equal(a[key], b[key])
    margin = min(a["margin"].min(), b["margin"].min())
    piv = np.concatenate([a["pivot"][np.isfinite(a["pivot"])], b["pivot"][np.isfinite(b["pivot"])]])
    near = (piv > 1e-14) & (piv < 1e-10)
    print(f"{what}: smallest |d^2 / thr^2 - 1| {margin:.2e}, lambda_2 / lambda_max in {piv.min() if len(piv) else np.nan:.2e} .. "
          f"{piv.max() if len(piv) else np.nan:.2e}")
    assert margin >= 1e-7 and not near.any()
    hc = a["hyp_count"]
    assert ((hc == -1) | (hc >= 8)).all()  # status 4 is a guard: a minimal sample fits its own 8 points


@pytest.mark.parametrize("name", sorted(RC.PARITY))
def test_parity_premises_and_host_versus_host_difference(name):
    a, b = RC.reference(name), RC.reference(name, "svd")
    _premises(a, b, name)
    ok = a["status"] == 0
    assert ok.all()
    d = np.abs(a["F"][ok] - b["F"][ok]).max()
    rel = (np.abs(a["quality"][ok, 0] - b["quality"][ok, 0]) / a["quality"][ok, 0]).max()
    dr = np.abs(a["quality"][ok, 1] - b["quality"][ok, 1]).max()
    print(f"{name}: eigh vs SVD max |dF| = {d:.3e} (recorded {RC.RANSAC_HOST_DIFF[name]:.1e}), Sampson RMS relative {rel:.3e}, ratio {dr:.3e}")
    assert 0.5 * RC.RANSAC_HOST_DIFF[name] <= d <= RC.RANSAC_HOST_DIFF[name]
    assert rel <= RC.MARGIN * RC.RANSAC_HOST_DIFF[name] and dr <= RC.MARGIN * RC.RANSAC_HOST_DIFF[name]
    F = a["F"][ok]
    np.testing.assert_allclose(np.linalg.norm(F, axis=(1, 2)), 1.0, rtol=0, atol=1e-14)
    assert (F.reshape(len(F), 9)[np.arange(len(F)), np.abs(F.reshape(len(F), 9)).argmax(axis=1)] > 0).all()
    # without refits the result is the best hypothesis itself: the same premises, the same statuses
    _premises(RC.reference(name, "eigh", 0), RC.reference(name, "svd", 0), name + ", n_refit = 0")


def test_status_cases_of_the_reference():
    for name, (pt_ptr, cam, xy, m, pairs, want) in RC.status_cases().items():
        a, b = (RR.two_view_robust(pt_ptr, cam, xy, m, pairs, RC.THRESHOLD, 16, 1, 2, lin) for lin in ("eigh", "svd"))
        _premises(a, b, name)
        assert a["status"].tolist() == [want], name
        if want:
            assert np.isnan(a["F"]).all() and np.isnan(a["quality"]).all() and not a["inlier"].any() and a["n_inliers"][0] == 0
    st = RC.status_cases()
    r = RR.two_view_robust(*st["eight"][:5], RC.THRESHOLD, 16, 1, 2)
    assert r["n_shared"][0] == 8 and (r["hyp_count"] == 8).all() and r["best"][0] == 0  # every hypothesis draws the same set
    r = RR.two_view_robust(*st["seven"][:5], RC.THRESHOLD, 16, 1, 2)
    assert r["n_shared"][0] == 7 and (r["hyp_count"] == -1).all() and r["best"][0] == -1
    r = RR.two_view_robust(*st["planar"][:5], RC.THRESHOLD, 16, 1, 2)
    assert r["n_shared"][0] == 80 and (r["hyp_count"] == -1).all()
    r = RR.two_view_robust(*st["all_replaced"][:5], RC.THRESHOLD, 16, 1, 2)
    assert r["n_shared"][0] == 80 and 8 <= r["n_inliers"][0] < 40  # (no geometry left: far below half of the shared points)


def test_reference_recovers_the_clean_points():
    """300x8 pair (0, 1), 30 % replaced: exactly the clean points, and the refit IS the fit of the clean points.  2000x3, 40 %
    replaced: no clean point is missed (some replaced ones lie within the threshold of their epipolar line by chance)."""
    pt_ptr, cam, xy, m, pairs, thr, H, seed, bad = RC.case("300x8")
    a = RC.reference("300x8")
    ids, xk, xl = T.shared(pt_ptr, cam, xy, 0, 1)
    assert len(ids) == 80 and bad.sum() == 24 and a["n_inliers"][0] == 56
    np.testing.assert_array_equal(a["inlier"][0][ids], ~bad)
    assert not a["inlier"][0][np.setdiff1d(np.arange(300), ids)].any()
    np.testing.assert_array_equal(a["F"][0], T.fundamental(xk[~bad], xl[~bad])[0])
    plain = T.fundamental(xk, xl)[0]
    print(f"300x8 (0, 1): plain fit is {np.abs(plain - a['F'][0]).max():.2f} from the clean F")
    assert np.abs(plain - a["F"][0]).max() > 0.5
    pt_ptr, cam, xy, m, pairs, thr, H, seed, bad = RC.case("2000x3")
    a = RC.reference("2000x3")
    ids, xk, xl = T.shared(pt_ptr, cam, xy, 0, 1)
    inl = a["inlier"][0]
    print(f"2000x3 (0, 1): {inl.sum()} inliers, {inl[bad].sum()} of them replaced points")
    assert inl[~bad].all() and inl.sum() == a["n_inliers"][0] == (~bad).sum() + inl[bad].sum() and inl[bad].sum() < 0.1 * bad.sum()
    clean = T.fundamental(xk[~bad], xl[~bad])[0]  # (entry-wise the two may differ by the sign rule: compare through the clean points)
    r_fit, r_clean = T.sampson_rms(a["F"][0], xk[~bad], xl[~bad]), T.sampson_rms(clean, xk[~bad], xl[~bad])
    assert r_clean <= r_fit <= 1.05 * r_clean, (r_fit, r_clean)
    conf = 1.0 - (1.0 - (a["n_inliers"] / a["n_shared"]) ** 8) ** H
    assert conf[0] > 0.8


def test_tile_arithmetic():
    assert RC.pair_tile(16641, 300, 8) == (128 << 20) // (48 * 16641 + 160 * 8) == 167
    assert RC.pair_tile(300, 30, 512) == 30 and RC.pair_tile(1 << 20, 1, 4096) == 1


def test_reference_pose_needs_the_robust_fit():
    """The conditions of the GPU relative_pose test: the robust pose on the contaminated pair is within POSE_FACTOR x the error
    the uncontaminated pair's pose has; the plain fit on the same data is not."""
    sc, xy, bad = RC.pose_case()
    (Ra, ta, Xa, ia), (Rb, tb, Xb, ib) = RC.reference_pose(), RC.reference_pose("svd")
    host = max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max())
    clean = T.relative_pose(sc.pt_ptr, sc.cam_idx, sc.xy, sc.K_gt, (0, 1))
    plain = T.relative_pose(sc.pt_ptr, sc.cam_idx, xy, sc.K_gt, (0, 1))
    e_clean, e_robust = RC.pose_error(sc, clean[0], clean[1]), RC.pose_error(sc, Ra, ta)
    e_plain = RC.pose_error(sc, plain[0], plain[1]) if plain[3]["status"] == 0 else np.inf
    print(f"pose: host-vs-host {host:.2e}, clean {e_clean:.2e}, robust {e_robust:.2e}, plain on the contaminated pair {e_plain:.2e}")
    assert ia["status"] == 0 and ia["n_inliers"] == 56 and sorted(ia["n_front"]) == [0, 0, 0, 56]
    assert np.isfinite(Xa).all(axis=1).sum() == 56 and np.array_equal(np.isfinite(Xa).all(axis=1), ia["inlier"])
    for got, rec in ((host, RC.POSE_HOST_DIFF), (e_clean, RC.POSE_CLEAN_ERR), (e_robust, RC.POSE_ROBUST_ERR), (e_plain, RC.POSE_PLAIN_ERR)):
        assert 0.5 * rec <= got <= rec, (got, rec)
    assert e_robust <= RC.POSE_FACTOR * e_clean < e_plain


def test_reference_bootstrap_registers_every_camera():
    """BOOT_FRACTION of camera 1's observations replaced, start pair (0, 1): the robust start and max_rms register all 8."""
    (R, t, X, info), (R2, t2, X2, i2) = RC.reference_bootstrap(), RC.reference_bootstrap(linear="svd")
    sc, xy, replaced = RC.bootstrap_case()
    assert info["camera_ok"].all() and sorted(info["order"]) == list(range(8)) and info["start_pair"] == (0, 1)
    np.testing.assert_array_equal(info["camera_ok"], i2["camera_ok"])
    np.testing.assert_array_equal(info["point_ok"], i2["point_ok"])
    ok = info["point_ok"]
    d = max(np.abs(R - R2).max(), np.abs(t - t2).max(), np.abs(X[ok] - X2[ok]).max())
    print(f"bootstrap: {replaced.sum()} observations replaced, {ok.sum()} points kept, host-vs-host {d:.2e} (recorded {RC.BOOT_HOST_DIFF:.1e})")
    assert 0.5 * RC.BOOT_HOST_DIFF <= d <= RC.BOOT_HOST_DIFF and ok.sum() >= 50


def _host_diff(a, b, name, scale_xy):
    """The eigh-versus-SVD figures of a case: max |dF| inside the 0.5x .. 1x bracket of its record, the Sampson RMS (relative
    to its own size; to the size of the observations where a minimal set is fitted exactly) and the ratio within the margin."""
    ok = a["status"] == 0
    d = np.abs(a["F"][ok] - b["F"][ok]).max()
    scale = np.where(a["n_inliers"][ok] > 8, a["quality"][ok, 0], scale_xy)
    rel = (np.abs(a["quality"][ok, 0] - b["quality"][ok, 0]) / scale).max()
    dr = np.abs(a["quality"][ok, 1] - b["quality"][ok, 1]).max()
    print(f"{name}: eigh vs SVD max |dF| = {d:.3e} (recorded {RC.RANSAC_HOST_DIFF[name]:.1e}), Sampson RMS relative {rel:.3e}, ratio {dr:.3e}")
    assert 0.5 * RC.RANSAC_HOST_DIFF[name] <= d <= RC.RANSAC_HOST_DIFF[name]
    assert rel <= RC.MARGIN * RC.RANSAC_HOST_DIFF[name] and dr <= RC.MARGIN * RC.RANSAC_HOST_DIFF[name]


@pytest.mark.parametrize("name", sorted(RC.LIMITS))
def test_limit_premises_and_host_versus_host_difference(name):
    """The structural limits of DESIGN.md §17: the premises of exact parity, the host-versus-host difference of the very case,
    and the structural premise that makes the case worth having -- asserted on the reference alone."""
    pt_ptr, cam, xy, m, pairs, thr, H, seed, n_refit = RC.limit_case(name)
    a, b = RC.limit_reference(name), RC.limit_reference(name, "svd")
    _premises(a, b, name)
    for key in ("n_accepted", "n_changed", "end"):
        np.testing.assert_array_equal(a[key], b[key])
    _host_diff(a, b, name, np.abs(xy).max())
    st, hc = a["status"], a["hyp_count"]
    print(f"{name}: status {st.tolist()}, accepted {a['n_accepted'].tolist()}, changed {a['n_changed'].tolist()}, end {a['end'].tolist()}")
    assert ((a["end"] == "") == (st != 0)).all() and (a["n_changed"] <= a["n_accepted"]).all() and (a["n_accepted"] <= n_refit).all()
    if name == "scan257":
        n_ch = -(-(len(pt_ptr) - 1) // 256)
        assert n_ch == 257 and -(-n_ch // 256) == 2  # per == 2: thread 128 owns one chunk, threads 129 .. 255 none
        cnt = RC.chunk_counts(pt_ptr, cam, xy, 0, 1)
        assert len(cnt) == 257 and {0, 1, 256} <= set(cnt.tolist()) and ((cnt > 1) & (cnt < 256)).any()
        assert cnt[0::4].tolist() == [256] * 64 + [164] and not cnt[1::4].any() and (cnt[2::4] == 1).all() and ((cnt[3::4] > 64) & (cnt[3::4] < 192)).all()
        assert (a["n_shared"] == cnt.sum()).all() and cnt.sum() % 256 != 0 and (st == 0).all()
        assert pairs.tolist() == [[0, 1], [1, 2], [2, 1]]
        # the two orders of a pair: other samples, other count tables, and -- here, at 16 refits -- one inlier set
        assert not np.array_equal(hc[1], hc[2]) and np.array_equal(a["inlier"][1], a["inlier"][2]) and a["end"].tolist() == ["exhausted"] * 3
    elif name == "refits_1.5e-3":
        assert (st == 0).all()
        assert ((a["n_changed"] >= 3) & (a["end"] == "rejected")).any()  # accepted changes, then a rejection: the other buffer is stale
        assert len(set(RC.end_refit(a, n_refit).tolist())) == 3  # the pairs of one tile leave RS_ACTIVE at three different refits
    elif name == "refits_3e-3":
        assert (st == 0).all() and (a["end"] == "exhausted").any() and (a["end"] == "rejected").any()
        assert ((a["end"] == "exhausted") & (a["n_changed"] >= 1) & (a["n_changed"] < a["n_accepted"])).any()  # a fixed point, kept to the end
    elif name == "mixed":
        assert st.tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 1, 0, 2, 0, 1, 0] and not a["n_shared"][st == 1].any()
        c = IC.COINCIDENT_CAMERA
        assert all(s == (1 if 8 in p else (2 if c in p else 0)) for p, s in zip(pairs.tolist(), st)) and [c, 0] in pairs.tolist() and [1, c] in pairs.tolist()
        assert (pairs[:, 0] > pairs[:, 1]).any() and (hc[st != 0] == -1).all() and (hc[st == 0] >= 8).all()
    elif name == "mixed65":
        ns = a["n_shared"]
        assert st.tolist() == [0, 1] * (len(st) // 2) and {1, 7} <= set(ns[1::2].tolist()) <= set(range(1, 8)) and (ns[0::2] >= 8).all()
    elif name == "partly_degenerate":
        assert st.tolist() == [0] and (hc == -1).any() and (hc >= 8).any() and a["best"][0] > 0 and hc[0, 0] == -1
        piv = a["pivot"][0]
        print(f"{name}: {(hc == -1).sum()} degenerate (lambda_2 / lambda_max <= {piv[hc[0] == -1].max():.1e}), {(hc >= 8).sum()} good (>= {piv[hc[0] >= 8].min():.1e}), best {a['best'][0]}")
    if name.startswith("refits"):  # the shorter loops the GPU test runs are prefixes of this one: their premises, their figures
        for r in RC.REFIT_COUNTS[:-1]:
            ar, br = RC.limit_reference(name, "eigh", r), RC.limit_reference(name, "svd", r)
            _premises(ar, br, f"{name}, n_refit = {r}")
            np.testing.assert_array_equal(ar["n_accepted"], np.minimum(a["n_accepted"], r))
            np.testing.assert_array_equal(ar["end"], np.where(RC.end_refit(a, n_refit) >= r, "exhausted", a["end"]))


def test_solver_failure_in_a_refit_is_not_reached():
    """No case of the suite ends a refit loop by a failure of the eigen-problem (DESIGN.md §17 says why none was built)."""
    for name in sorted(RC.LIMITS):
        assert "solver" not in RC.limit_reference(name)["end"].tolist(), name


def test_maximum_hypothesis_count_premises():
    """n_hypotheses = 65 536 on "300x8" pair (0, 1): the hypotheses the GPU test compares meet the premises of exact counts, and
    the helper that evaluates single h is the table of the full call."""
    (hs, ca, ma, pa), (_, cb, mb, pb) = RC.max_hyp_reference(), RC.max_hyp_reference("svd")
    assert hs[1] == 97 and hs[-64] == RC.MAX_HYP - 64 and hs[-1] == RC.MAX_HYP - 1 and len(hs) == 676 + 64 - 1  # (65 475 is in both)
    np.testing.assert_array_equal(ca, cb)
    piv = np.concatenate([pa, pb])
    print(f"H = 65536 sample: smallest |d^2 / thr^2 - 1| {min(ma, mb):.2e}, lambda_2 / lambda_max in {piv.min():.2e} .. {piv.max():.2e}")
    assert min(ma, mb) >= 1e-7 and not ((piv > 1e-14) & (piv < 1e-10)).any() and (ca >= 8).all()
    full = RC.reference("300x8")["hyp_count"][0]  # H = 512
    low = hs[hs < 512]
    np.testing.assert_array_equal(ca[: len(low)], full[low])
