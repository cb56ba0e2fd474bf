"""Robust resection, the part that needs no GPU: the sample generator libmvba.so exports is the reference's and
the first 6 draws of the two-view one, the premises under which the GPU parity tests may ask for EXACT count tables hold on
every case, the reference recovers the clean observations, and the host-versus-host differences that set the GPU margins are
what tests/_resect_ransac_cases.py records."""
import ctypes
import os

import numpy as np
import pytest

import _init_cases as IC
import _resect_ransac_cases as QC
import _resect_ransac_ref as QR
from lib import _mvba
from lib.initialization import ransac_sample, resect_sample

SAMPLE_TABLE = [(0, 0, 0, 6), (0, 0, 0, 7), (1, 0, 5, 80), (1, 3, 511, 157), ((1 << 64) - 1, 3, 7, (1 << 31) - 1), (7, 5, 511, 300),
                (1, 1703, 65535, 9), (12345678901234567890, 6, 3, 8)]


@pytest.mark.parametrize("seed,k,h,n", SAMPLE_TABLE)
def test_exported_sample_generator_is_the_reference(seed, k, h, n):
    """n = 6 (a permutation), n = 7 (below the two-view generator's range), n = 2^31 - 1, seed = 2^64 - 1."""
    got, want = resect_sample(seed, k, h, n), QR.sample(seed, k, h, n)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int64 and len(set(got.tolist())) == 6 and (got >= 0).all() and (got < n).all()
    if n == 6:
        assert sorted(got.tolist()) == list(range(6))
    if n >= 8:  # the 8-draw instance is unchanged, and the 6 draws are its first 6
        np.testing.assert_array_equal(got, ransac_sample(seed, k, k, h, n)[:6])


def test_sample_depends_on_camera_and_seed_and_rejects_bad_arguments():
    assert not np.array_equal(resect_sample(1, 0, 5, 80), resect_sample(1, 1, 5, 80))
    assert not np.array_equal(resect_sample(1, 0, 5, 80), resect_sample(2, 0, 5, 80))
    for args, text in (((0, 0, 0, 5), "n = 5"), ((0, 0, 0, 1 << 31), "n = 2147483648"), ((0, 0, -1, 80), "h = -1"), ((0, -2, 0, 80), "k = -2")):
        with pytest.raises(ValueError, match=text):
            resect_sample(*args)


def test_library_exports_the_entry_points_and_checks_arguments_without_a_device():
    assert "mvba_resect_robust" in _mvba.SIGNATURES and "mvba_resect_sample" in _mvba.SIGNATURES
    lib = ctypes.CDLL(_mvba.LIB_PATH)
    for name in ("mvba_resect_robust", "mvba_resect_sample"):
        assert hasattr(lib, name), name
    lib = _mvba.load_library()
    i32, i64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    X, pt_ptr, cam, xy, m, _ = IC.resect_case("300x8")
    X, xy, P = np.ascontiguousarray(X), np.ascontiguousarray(xy), np.empty((8, 12))

    def call(thr=0.01, H=16, n_refit=2, cameras=None, nc=None):
        cams = None if cameras is None else np.asarray(cameras, np.int32)
        rc = lib.mvba_resect_robust(_mvba._ptr(X), 300, pt_ptr.ctypes.data_as(i64), cam.ctypes.data_as(i32), _mvba._ptr(xy), len(cam), m, None,
                                    None if cams is None else cams.ctypes.data_as(i32), (m if cams is None else len(cams)) if nc is None else nc,
                                    thr, H, 1, n_refit, _mvba._ptr(P), None, None, None, None, None, None, None, None, -1)
        return rc, lib.mvba_last_error().decode()

    for kw, text in (({"thr": 0.0}, "threshold = 0.0"), ({"thr": float("nan")}, "threshold = nan"), ({"thr": -0.5}, "threshold = -0.5"),
                     ({"H": 0}, "n_hypotheses = 0"), ({"H": 65537}, "n_hypotheses = 65537"), ({"n_refit": -1}, "n_refit = -1"),
                     ({"n_refit": 17}, "n_refit = 17"), ({"cameras": [5, 8]}, "cameras[1] = 8"), ({"cameras": [-1]}, "cameras[0] = -1"),
                     ({"nc": -1}, "n_cameras = -1"), ({"nc": 3}, "n_cameras = 3 must be n_images = 8")):
        rc, msg = call(**kw)
        assert rc == _mvba.MVBA_ERR_BADARG and text in msg, (kw, msg)


def test_resect_robust_fails_loudly_without_gpu():
    if os.path.exists(_mvba.LIB_PATH) and _mvba.device_count() > 0:
        pytest.skip("a device is visible")
    X, pt_ptr, cam, xy, m, _ = IC.resect_case("300x8")
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        _mvba.resect_robust(X, pt_ptr, cam, xy, m, 0.01)


def _premises(a, b, what):
    """(a) eigh and SVD null vectors give one count table (and everything that follows from it); (b) no distance within 1e-7
    (relative, squared) of the threshold; (c) no hypothesis within a factor 100 of the pivot rule."""
    for key in ("hyp_count", "status", "best", "n_inliers", "inlier", "n_usable", "sizes", "end"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    margin = min(a["margin"].min(), b["margin"].min())
    piv = np.concatenate([a["pivot"][np.isfinite(a["pivot"])], b["pivot"][np.isfinite(b["pivot"])]])
    near = (piv > 1e-14) & (piv < 1e-10)
    print(f"{what}: smallest |d^2 / thr^2 - 1| {margin:.2e}, lambda_2 / lambda_max in {piv.min() if len(piv) else np.nan:.2e} .. "
          f"{piv.max() if len(piv) else np.nan:.2e}")
    assert margin >= 1e-7 and not near.any()


def _host_difference(a, b, what, recorded):
    ok = a["status"] == 0
    d = np.abs(a["P"][ok] - b["P"][ok]).max()
    dq = np.abs(a["quality"][ok] - b["quality"][ok]).max(axis=0)
    print(f"{what}: eigh vs SVD max |dP| = {d:.3e} (recorded {recorded:.1e}), RMS {dq[0]:.3e}, ratio {dq[1]:.3e}")
    assert 0.5 * recorded <= d <= recorded
    assert dq[0] <= QC.MARGIN * recorded and dq[1] <= QC.MARGIN * recorded
    P = a["P"][ok]
    np.testing.assert_allclose(np.linalg.norm(P[:, 2, :3], axis=1), 1.0, rtol=0, atol=1e-14)
    assert (np.linalg.det(P[:, :, :3]) > 0).all()
    bad = ~ok
    assert np.isnan(a["P"][bad]).all() and np.isnan(a["quality"][bad]).all() and (a["n_inliers"][bad] == 0).all()


@pytest.mark.parametrize("name", sorted(QC.PARITY))
def test_parity_premises_and_host_versus_host_difference(name):
    a, b = QC.reference(name), QC.reference(name, "svd")
    _premises(a, b, name)
    _host_difference(a, b, name, QC.RESECT_RANSAC_HOST_DIFF[name])
    if name == "300x8":  # without refits the result is the best hypothesis itself
        a0, b0 = QC.reference(name, "eigh", 0), QC.reference(name, "svd", 0)
        _premises(a0, b0, name + ", n_refit = 0")
        _host_difference(a0, b0, name + ", n_refit = 0", QC.RESECT_RANSAC_HOST_DIFF["300x8_refit0"])
        np.testing.assert_array_equal(a0["n_inliers"], a0["hyp_count"].max(axis=1))
        assert (a0["quality"][:, 1] == 0).all()


def test_status_shapes_of_the_reference():
    for name in QC.STATUS_NAMES:
        a, b = QC.status_reference(name), QC.status_reference(name, "svd")
        _premises(a, b, name)
        want = QC.status_case(name)[6]
        if want is not None:
            if name == "empty":  # (16 hypotheses: a camera may end with status 4; the unobserved ones have status 1)
                assert (a["status"][list(IC.EMPTY_CAMERAS)] == 1).all() and (a["n_usable"][list(IC.EMPTY_CAMERAS)] == 0).all()
            else:
                np.testing.assert_array_equal(a["status"], want, err_msg=name)
        if name != "coplanar":
            _host_difference(a, b, name, QC.RESECT_RANSAC_HOST_DIFF[name])
    r = QC.status_reference("six")
    assert r["n_usable"].tolist() == [60, 6, 5, 60] and (r["hyp_count"][1] == 6).all() and r["best"][1] == 0 and r["n_inliers"][1] == 6
    assert (r["hyp_count"][2] == -1).all() and r["best"][2] == -1
    r = QC.status_reference("coplanar")
    assert (r["hyp_count"] == -1).all() and (r["best"] == -1).all() and not r["inlier"].any() and np.isnan(r["P"]).all()
    r = QC.status_reference("empty")
    assert (r["hyp_count"][list(IC.EMPTY_CAMERAS)] == -1).all()
    # the usable filter: by point_ok, or by NaN in X -- one result
    a, b = QC.status_reference("point_ok"), QC.status_reference("nan_X")
    for key in ("P", "quality", "hyp_count", "inlier", "n_usable", "n_inliers"):
        np.testing.assert_array_equal(a[key], b[key])
    assert (a["n_usable"] < QC.reference("300x8")["n_usable"]).all()
    # no geometry left in camera 3: status 4 here (unlike the 8-point F, a minimal 6-point DLT has 12 rows for 11 unknowns and
    # does not fit its own sample exactly, so a count below 6 can be reached from data), or a count far below half
    r = QC.status_reference("all_replaced")
    c = QC.ALL_REPLACED_CAMERA
    assert r["status"][c] == 4 and 0 <= r["hyp_count"][c].max() < 6 and r["best"][c] >= 0 and r["n_inliers"][c] == 0


def test_reference_recovers_the_clean_observations():
    """300x8, 30 % of every camera's observations replaced: the inliers are exactly the clean observations for every camera
    (camera 1's best minimal sample counts 117, one replaced observation within the threshold by chance; its first refit has
    116 -- the two-view rule would have stopped there with the minimal-sample P), and the refit IS the fit of the clean set."""
    X, pt_ptr, cam, xy, m, thr, H, seed, _, hit = QC.case("300x8")
    a = QC.reference("300x8")
    np.testing.assert_array_equal(a["inlier"], ~hit)
    assert a["sizes"][1].tolist() == [117, 116, 116] and a["n_accepted"][1] == 2
    pt = np.repeat(np.arange(len(X)), np.diff(pt_ptr))
    clean = IC.ref.resect(X, pt_ptr[: len(X) + 1], cam, xy, m)[0]  # plain resection of everything: moved by the replaced observations
    for k in range(m):
        sel = (cam == k) & ~hit
        Pk = IC.ref.resect_camera(X[pt[sel]], xy[sel])[0]
        np.testing.assert_array_equal(a["P"][k], Pk)
        assert np.abs(clean[k].reshape(3, 4) - Pk).max() > 1.0
    a0 = QC.reference("300x8", "eigh", 0)
    d0 = np.abs(a0["P"][1] - a["P"][1]).max()
    print(f"camera 1: the minimal-sample P is {d0:.2f} from the clean fit")
    assert d0 > 0.1


def test_refit_trace_of_the_reference():
    """"5000x3" at twice the noise: every refit moves the inlier set; at 16 the loop ends by rejection after 5, 5 and 6."""
    for r in QC.REFIT_COUNTS:
        a, b = QC.refit_reference(r), QC.refit_reference(r, "svd")
        _premises(a, b, f"refits, n_refit = {r}")
        _host_difference(a, b, f"refits, n_refit = {r}", QC.REFIT_HOST_DIFF[r])
        assert (a["n_accepted"] == a["n_changed"]).all()
    assert (QC.refit_reference(2)["n_accepted"] == 2).all()
    a = QC.refit_reference(16)
    assert a["n_accepted"].tolist() == [5, 5, 6] and (a["end"] == "rejected").all()
    # the first refit needs 6 inliers of its own, not the best count; the refit that ends the loop shrank the set
    s = a["sizes"]
    assert (s[:, 1] >= 6).all() and all(s[k, a["n_accepted"][k] + 1] < s[k, a["n_accepted"][k]] for k in range(3))


def test_max_hypotheses_sample_premises():
    hs, c, margin, pivot = QC.max_hyp_reference()
    hs2, c2, margin2, pivot2 = QC.max_hyp_reference("svd")
    np.testing.assert_array_equal(c, c2)
    piv = np.concatenate([pivot, pivot2])
    assert min(margin, margin2) >= 1e-7 and not ((piv > 1e-14) & (piv < 1e-10)).any() and len(hs) == 739 and (c >= 0).all()


def test_camera_tiles():
    """The documented tile formula, restated in Python, at the sizes the GPU tests rely on (the C code's own tile size is not
    observable from outside: see QC.camera_tile)."""
    assert QC.camera_tile(300, 64) == 300 and QC.camera_tile(300, 8192) == 163 and QC.camera_tile(8, 65536) == 8 and QC.camera_tile(100, 512) == 100


def test_bootstrap_reference_on_contaminated_tracks():
    """What the feature buys, on the host: 20 % of the observations of cameras 2 .. 7 replaced.  The robust bootstrap registers 8
    cameras with poses within BOOT_FACTOR of the uncontaminated run's error and uses no replaced observation; the plain one
    registers 4, two of them wrong by more than 1."""
    sc, xy, hit = QC.bootstrap_case()
    assert hit.sum() == 207
    (Ra, ta, Xa, ia), (Rb, tb, Xb, ib) = QC.reference_bootstrap(), QC.reference_bootstrap("svd")
    assert ia["order"] == ib["order"] == [0, 1, 2, 7, 6, 3, 5, 4] and ia["camera_ok"].all()
    for key in ("point_ok", "obs_ok", "inlier"):
        np.testing.assert_array_equal(ia[key], ib[key])
    ok = ia["point_ok"]
    d = max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max(), np.abs(Xa[ok] - Xb[ok]).max())
    clean = QC.plain_bootstrap(False)
    e_clean, e_robust = max(QC.pose_error(sc, clean[0], clean[1], clean[3]["camera_ok"])), max(QC.pose_error(sc, Ra, ta, ia["camera_ok"]))
    print(f"robust bootstrap: {ok.sum()} points, host difference {d:.3e} (recorded {QC.BOOT_HOST_DIFF:.1e}), pose error {e_robust:.3e} "
          f"(recorded {QC.BOOT_ROBUST_ERR:.1e}), uncontaminated {e_clean:.3e} (recorded {QC.BOOT_CLEAN_ERR:.1e})")
    assert ok.sum() == 251 and clean[3]["camera_ok"].all()
    assert 0.5 * QC.BOOT_HOST_DIFF <= d <= QC.BOOT_HOST_DIFF
    assert 0.9 * QC.BOOT_CLEAN_ERR <= e_clean <= QC.BOOT_CLEAN_ERR and 0.9 * QC.BOOT_ROBUST_ERR <= e_robust <= QC.BOOT_ROBUST_ERR
    assert e_robust <= QC.BOOT_FACTOR * e_clean
    assert not (ia["inlier"] & hit).any() and not (ia["inlier"] & ~ia["obs_ok"]).any() and (hit & ~ia["obs_ok"]).sum() > 100
    plain = QC.plain_bootstrap(True)
    assert plain[3]["camera_ok"].sum() == 4 and max(QC.pose_error(sc, plain[0], plain[1], plain[3]["camera_ok"])) > 1.0


def test_tiles_edges_premises_and_what_a_wrong_chunk_offset_would_return():
    """The DLT tile case of tests/test_gpu_pose_limits.py: seven times the "edges" list at 65 536 hypotheses is 21
    entries for a tile of 20, and entry 20 starts at chunk 27.  A tile loop that put the second tile's chunk partials at the camera
    offset would hand entry 20 another sum: the expected n_inliers changes."""
    cams, H = list(QC.TILE_CAMERAS), QC.TILE_HYP
    a = QC.reference("edges_h65")
    tile, lc = QC.camera_tile(len(cams), H), QC.list_chunks(cams, a["n_usable"])
    assert tile == 20 and len(cams) == 21 and lc[20] == 27 != 20 and lc[-1] == 28 and (a["status"] == 0).all()
    cam = QC.case("edges_h65")[2]
    masks = [a["inlier"][cam == k] for k in range(3)]
    want = a["n_inliers"][cams]
    np.testing.assert_array_equal(QC.tile_sums(cams, a["n_usable"], masks, tile), want)
    wrong = QC.tile_sums(cams, a["n_usable"], masks, tile, offset="camera")
    assert (wrong[:20] == want[:20]).all() and wrong[20] != want[20]
