"""Similarity alignment on the device: mvba_align_robust and mvba_align against the NumPy restatement of
tests/_align_ref.py -- integers exactly (the premises are asserted by test_align_cpu.py), (s, Q, tau) and quality within MARGIN x the
recorded host-versus-host figure --, their structural limits, and a bootstrap brought into the frame of its control points."""
import numpy as np
import pytest

import _align_cases as AC
import _align_ref as AR
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster
from lib.initialization import align_to_control_points, bootstrap, fit_similarity, robust_similarity

pytestmark = pytest.mark.gpu

KEYS = ("s", "Q", "tau", "quality", "n_usable", "n_inliers", "best", "status", "inlier", "hyp_count")


def _run(src, dst, thr, ok=None, with_scale=True, H=512, seed=0, n_refit=2):
    return _mvba.align_robust(src, dst, thr, ok=ok, with_scale=with_scale, n_hypotheses=H, seed=seed, n_refit=n_refit, return_counts=True)


def _sim13(got):
    return np.concatenate([[got["s"]], got["Q"].ravel(), got["tau"]])


def _assert_exact(got, want, what):
    for key in ("hyp_count", "inlier"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")
    for key in ("best", "n_usable", "n_inliers", "status"):
        assert got[key] == want[key], f"{what}: {key}"


def _assert_close(got, want, name, what):
    """(s, Q, tau) within MARGIN x the case's figure, the RMS within rms_margin, gap and spread within the margin relative to their
    size; where the status is not 0: NaN, no inliers."""
    if want["status"] != 0:
        assert np.isnan(_sim13(got)).all() and np.isnan(got["quality"]).all() and not got["inlier"].any() and got["n_inliers"] == 0
        return
    margin = AC.MARGIN * AC.HOST_DIFF[name]
    d = np.abs(_sim13(got) - want["sim13"]).max()
    rms = abs(got["quality"][0] - want["quality"][0])
    big = np.maximum(np.abs(want["quality"][1:]), 1.0 if want["quality"][1] == 0.0 else 0.0)
    rel = (np.abs(got["quality"][1:] - want["quality"][1:]) / big).max()
    print(f"{what}: max |d(s, Q, tau)| {d:.3e} (margin {margin:.1e}), RMS {rms:.3e} (margin {AC.rms_margin(name):.1e}), gap and spread relative {rel:.3e}")
    assert d <= margin and rms <= AC.rms_margin(name) and rel <= margin
    assert abs(np.linalg.det(got["Q"]) - 1.0) <= 1e-14 and np.abs(got["Q"] @ got["Q"].T - np.eye(3)).max() <= 1e-14


def _assert_same(a, b, what, keys=KEYS):
    for key in keys:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), f"{what}: {key}"


@pytest.mark.parametrize("name", sorted(AC.PARITY))
def test_parity_with_the_reference(name):
    """80 rows (one chunk), 257 (two chunks, the last of one row), 300, the rigid twin, an ok mask with NaN rows; two calls bitwise;
    without refits the inliers are those of the best hypothesis."""
    src, dst, ok, ws, thr, H, seed, clean = AC.case(name)
    got, want = _run(src, dst, thr, ok, ws, H, seed), AC.reference(name)
    _assert_exact(got, want, name)
    _assert_close(got, want, name, name)
    np.testing.assert_array_equal(got["inlier"], clean)
    _assert_same(got, _run(src, dst, thr, ok, ws, H, seed), f"{name}: two calls")
    zero = _run(src, dst, thr, ok, ws, H, seed, 0)
    _assert_exact(zero, AC.reference(name, "horn", 0), name + ", n_refit = 0")
    assert zero["n_inliers"] == want["hyp_count"].max() and zero["quality"][1] == 0.0
    if not ws:
        assert got["s"] == 1.0 and zero["s"] == 1.0


@pytest.mark.parametrize("name", sorted(AC.PARITY))
def test_plain_fit_against_the_reference(name):
    """mvba_align on the clean rows; two calls bitwise; unchanged, bit for bit, when unusable rows are interleaved."""
    src, dst, _, ws, _, _, _, clean = AC.case(name)
    x, y = src[clean], dst[clean]
    got, want = _mvba.align(x, y, with_scale=ws), AC.plain_reference(name)
    assert got["status"] == 0 and got["n_usable"] == clean.sum()
    _assert_close(got, want, name, name + ", plain")
    keys = ("s", "Q", "tau", "quality", "n_usable", "status")
    _assert_same(got, _mvba.align(x, y, with_scale=ws), f"{name}: two calls", keys)
    s2, d2, o2, _ = AC.interleave_nan(x, y)
    _assert_same(got, _mvba.align(s2, d2, ok=o2, with_scale=ws), f"{name}: NaN rows interleaved", keys)
    s2[~o2] = 7.0  # the same rows finite, forbidden by ok alone
    d2[~o2] = -7.0
    _assert_same(got, _mvba.align(s2, d2, ok=o2, with_scale=ws), f"{name}: forbidden rows interleaved", keys)
    s, Q, tau, info = fit_similarity(x, y, with_scale=ws)
    assert s == got["s"] and np.array_equal(Q, got["Q"]) and np.array_equal(tau, got["tau"]) and info["status"] == 0


@pytest.mark.parametrize("H", AC.LIMIT_H)
def test_hypothesis_block_boundaries(H):
    """One hypothesis (status 4: its sample holds a replaced row and counts nothing), a full LDS block, and a second block of one."""
    src, dst, ok, ws, thr, _, seed, _ = AC.case("a80")
    got, want = _run(src, dst, thr, ok, ws, H, seed), AC.reference("a80", n_hyp=H)
    _assert_exact(got, want, f"H = {H}")
    _assert_close(got, want, f"h{H}", f"H = {H}")
    assert got["hyp_count"].shape == (H,)
    if H == 1:
        assert got["status"] == 4 and got["best"] == 0 and got["hyp_count"][0] == 0


def test_minimum_row_counts_and_degenerate_input():
    """Exactly three usable rows: status 0, every count 3; two: status 1; src on a line, exactly: status 2, from mvba_align too; none
    of it changed by NaN rows behind ok."""
    thr = AC.THRESHOLD * AC.SCALE
    src, dst, ok = AC.few_case(3)
    got, want = _run(src, dst, thr, ok, True, 64, 1), AR.align_robust(src, dst, thr, ok, True, 64, 1, 2)
    _assert_exact(got, want, "three")
    _assert_close(got, want, "three", "three")
    assert got["status"] == 0 and (got["hyp_count"] == 3).all() and got["n_usable"] == 3 and got["n_inliers"] == 3 and got["best"] == 0
    src, dst, ok = AC.few_case(2)
    got = _run(src, dst, thr, ok, True, 64, 1)
    assert got["status"] == 1 and got["n_usable"] == 2 and (got["hyp_count"] == -1).all() and got["best"] == -1
    assert np.isnan(_sim13(got)).all() and np.isnan(got["quality"]).all() and not got["inlier"].any()
    assert _mvba.align(src, dst, ok=ok)["status"] == 1
    none = _run(src, dst, thr, np.zeros(len(src), bool), True, 64, 1)
    assert none["status"] == 1 and none["n_usable"] == 0 and none["best"] == -1
    src, dst = AC.collinear_case()
    got = _run(src, dst, thr, None, True, 64, 1)
    assert got["status"] == 2 and got["n_usable"] == 80 and (got["hyp_count"] == -1).all() and got["best"] == -1 and got["n_inliers"] == 0
    assert np.isnan(_sim13(got)).all() and not got["inlier"].any()
    plain = _mvba.align(src, dst)
    assert plain["status"] == 2 and plain["n_usable"] == 80 and np.isnan(plain["s"]) and _mvba.align(dst, src)["status"] == 2
    s2, d2, o2, pos = AC.interleave_nan(src, dst)
    got2 = _run(s2, d2, thr, o2, True, 64, 1)
    assert got2["status"] == 2 and got2["n_usable"] == 80 and (got2["hyp_count"] == -1).all()
    src, dst, ok = AC.few_case(3)
    s2, d2, o2, pos = AC.interleave_nan(src, dst, ok)
    got3 = _run(s2, d2, thr, o2, True, 64, 1)
    assert got3["status"] == 0 and got3["n_usable"] == 3 and got3["inlier"].sum() == 3 and got3["inlier"][pos[ok]].all()


@pytest.mark.parametrize("n", AC.SCAN_SIZES)
def test_chunk_scan(n):
    """256, 257 and 513 rows under an ok mask: whole chunks, a chunk of one row, a chunk without a usable row."""
    src, dst, ok = AC.scan_case(n)
    got, want = _run(src, dst, AC.THRESHOLD * AC.SCALE, ok, True, 64, 1), AC.scan_reference(n)
    _assert_exact(got, want, f"scan {n}")
    _assert_close(got, want, f"scan{n}", f"scan {n}")
    assert not got["inlier"][~ok].any()


@pytest.mark.parametrize("n_refit", AC.REFIT_COUNTS)
def test_refits_move_the_inlier_set(n_refit):
    src, dst, ok, ws, _, H, seed, _ = AC.case("a80")
    got, want = _run(src, dst, AC.REFIT_THRESHOLD, ok, ws, H, seed, n_refit), AC.refit_reference(n_refit)
    _assert_exact(got, want, f"n_refit = {n_refit}")
    _assert_close(got, want, "refits", f"n_refit = {n_refit}")


def test_maximum_hypothesis_count():
    """n_hypotheses = 65 536 on the 80-row case: 1024 hypothesis blocks; the sampled entries of the table."""
    src, dst, ok, ws, thr, _, seed, _ = AC.case("a80")
    got = _run(src, dst, thr, ok, ws, AC.MAX_HYP, seed)
    hs, counts, _, _ = AC.max_hyp_reference()
    np.testing.assert_array_equal(got["hyp_count"][hs], counts)
    assert got["status"] == 0 and got["hyp_count"].shape == (AC.MAX_HYP,) and got["n_inliers"] == AC.N_CLEAN["a80"]
    assert got["best"] == int(np.argmax(got["hyp_count"]))


def test_python_surface():
    src, dst, ok, ws, thr, H, seed, clean = AC.case("masked300")
    s, Q, tau, info = robust_similarity(src, dst, thr, ok=ok, n_hypotheses=H, seed=seed)
    got = _run(src, dst, thr, ok, ws, H, seed)
    assert s == got["s"] and np.array_equal(Q, got["Q"]) and np.array_equal(tau, got["tau"])
    np.testing.assert_array_equal(info["inlier"], clean)
    w = info["n_inliers"] / info["n_usable"]
    assert info["confidence"] == pytest.approx(1.0 - (1.0 - w ** 3) ** H, abs=1e-15) and set(info["timings_ms"]) == {"upload", "score", "refit", "other"}


CONTROL_THRESHOLD = 0.1  # units of the survey: a 30th of the scene's unit (the surveyed frame is the ground truth's scaled by 3)


def test_bootstrap_into_the_frame_of_its_control_points_then_held_bundle_adjustment():
    """bootstrap on the 300 x 8 scene (camera 0 at the origin, unit baseline), 40 of its points surveyed in the ground-truth frame
    scaled by 3, 12 of them with wrong coordinates: align_to_control_points holds exactly the 28 others and lands where the
    reference's alignment of the same data lands; the BA from there keeps the held rows bit for bit and ends no farther from the
    scaled ground truth than the same BA started from the reference's least-squares similarity over the 28 clean control points.
    The host-versus-host figures (horn against svd, on the bootstrap's output, which exists on the device alone) are taken here and
    floored at the rounding of a coordinate: eps x CONTROL_SCALE.  (Measured: the held BA ends at 3.50e-2 from the scaled ground truth
    where the alignment alone stood at 3.29e-2 -- camera 0 keeps the pose the alignment gave it, error included, against 28 points
    held at their surveyed positions: the limit DESIGN.md 21 records.  Printed, not asserted.)"""
    from lib.synthetic import make_scene

    sc = make_scene(300, 8, vis_p=0.5)
    K, R, t, X, bi = bootstrap(sc.pt_ptr, sc.cam_idx, sc.xy, sc.init_K)
    assert bi["camera_ok"].all() and bi["point_ok"].all()  # (bootstrap keeps every point of this scene: the list needs no restriction)
    ids, xyz, wrong = AC.control_points(sc, bi["point_ok"])
    world, floor = AC.CONTROL_SCALE * sc.X_gt, np.finfo(float).eps * AC.CONTROL_SCALE
    Xa, Ra, ta, info = align_to_control_points(X, R, t, ids, xyz, CONTROL_THRESHOLD, seed=1)
    refs = [AR.align_robust(X[ids], xyz, CONTROL_THRESHOLD, None, True, 512, 1, 2, route) for route in AR.ROUTES]
    for a in refs:  # the premises, on this data
        assert a["status"] == 0 and a["margin"] >= AC.GUARD and np.array_equal(a["inlier"], ~wrong)
    assert info["status"] == 0 and info["n_inliers"] == AC.N_CONTROL - AC.N_WRONG
    np.testing.assert_array_equal(info["held"], ids[~wrong])
    np.testing.assert_array_equal(info["hyp_count"], refs[0]["hyp_count"])
    np.testing.assert_array_equal(Xa[info["held"]], xyz[~wrong])
    # where the alignment lands: cameras and free points against the scaled ground truth, as the reference's does
    free = bi["point_ok"].copy()
    free[info["held"]] = False

    def distance(Xq, tq):
        return np.sqrt(((Xq[free] - world[free]) ** 2).sum(axis=1).mean()), np.sqrt(((tq - AC.CONTROL_SCALE * sc.t_gt) ** 2).sum(axis=1).mean())

    (Xh, Rh, th), (Xs, Rs, ts) = (AR.transform(a["sim13"], X, R, t) for a in refs)
    got, horn, svd = distance(Xa, ta), distance(Xh, th), distance(Xs, ts)
    margin = AC.MARGIN * max(abs(horn[0] - svd[0]), abs(horn[1] - svd[1]), floor)
    print(f"aligned: free points {got[0]:.6e} (reference {horn[0]:.6e}), camera centres {got[1]:.6e} (reference {horn[1]:.6e}) from the scaled ground "
          f"truth; margin {margin:.1e}; s = {info['s']:.4f}")
    assert got[0] <= horn[0] + margin and got[1] <= horn[1] + margin
    assert max(np.abs(Xa[free] - Xh[free]).max(), np.abs(Ra - Rh).max(), np.abs(ta - th).max()) <= AC.MARGIN * max(
        np.abs(Xh[free] - Xs[free]).max(), np.abs(Rh - Rs).max(), np.abs(th - ts).max(), floor)

    def adjust(X0, R0, t0):
        X0 = X0.copy()
        X0[info["held"]] = xyz[~wrong]
        ba = BundleAdjuster.from_observations(sc.n_points, 8, sc.pt_ptr, sc.cam_idx, sc.xy, X0, K, R0, t0, axis=bi["axis"], hold_points=info["held"])
        Xb = ba.optimize()[0]
        assert Xb[info["held"]].tobytes() == xyz[~wrong].tobytes()
        return np.sqrt(((Xb[free] - world[free]) ** 2).sum(axis=1).mean())

    e_got, e_horn, e_svd = adjust(Xa, Ra, ta), adjust(Xh, Rh, th), adjust(Xs, Rs, ts)
    margin = AC.MARGIN * max(abs(e_horn - e_svd), floor)
    print(f"after the held BA: free points {e_got:.6e} from the scaled ground truth (reference start {e_horn:.6e}, svd start {e_svd:.6e}; "
          f"before: {got[0]:.6e}); margin {margin:.1e}")
    assert e_got <= e_horn + margin
