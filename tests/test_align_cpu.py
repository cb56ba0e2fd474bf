"""Similarity alignment, the part that needs no GPU: the sample generator and the entry points libmvba.so exports,
the premises under which the GPU parity tests may ask for EXACT integers, what the reference recovers from contaminated
correspondences, transform_reconstruction, and the host-versus-host differences that set the GPU margins -- all of them what
tests/_align_cases.py records."""
import ctypes
import os

import numpy as np
import pytest

import _align_cases as AC
import _align_ref as AR
from lib import _mvba
from lib.initialization import align_sample, ransac_sample, transform_reconstruction
from lib.synthetic import make_scene, project_obs

SAMPLE_TABLE = [(0, 0, 3), (1, 5, 80), (1, 511, 80), ((1 << 64) - 1, 7, (1 << 31) - 1), (7, 511, 300), (1, 65535, 5), (12345678901234567890, 3, 8),
                (1, 5, 7), (3, 2147483647, 257)]


@pytest.mark.parametrize("seed,h,n", SAMPLE_TABLE)
def test_exported_sample_generator_is_the_reference(seed, h, n):
    """n = 3 (a permutation), n below 8 (which mvba_ransac_sample refuses), n = 2^31 - 1, seed = 2^64 - 1, h = 2^31 - 1; and for
    n >= 8 the first three draws of the 8-point sampler of pair (0, 0)."""
    got, want = align_sample(seed, h, n), AR.sample(seed, h, n)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int64 and len(set(got.tolist())) == 3 and (got >= 0).all() and (got < n).all()
    if n == 3:
        assert sorted(got.tolist()) == [0, 1, 2]
    if n >= 8:
        np.testing.assert_array_equal(got, ransac_sample(seed, 0, 0, h, n)[:3])


def test_sample_rejects_bad_arguments():
    with pytest.raises(ValueError, match="n = 2 "):
        align_sample(0, 0, 2)
    with pytest.raises(ValueError, match="h = -1"):
        align_sample(0, -1, 80)
    with pytest.raises(ValueError, match="n = 2147483648 must be in 3"):
        align_sample(0, 0, 1 << 31)


def test_library_exports_the_alignment_entry_points():
    """The new symbols exist with bound prototypes; argument errors come before any device work and name the number."""
    names = ("mvba_align_robust", "mvba_align", "mvba_align_sample")
    for name in names:
        assert name in _mvba.SIGNATURES, name
    raw = ctypes.CDLL(_mvba.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), name
    lib = _mvba.load_library()
    for name in names:
        res, args = _mvba.SIGNATURES[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args
    src, dst = (np.ascontiguousarray(a) for a in AC.case("a80")[:2])
    sim = np.empty(13)

    def call(n=80, thr=0.01, H=16, n_refit=2, a=src, b=dst, out=sim):
        p = [None if v is None else _mvba._ptr(v) for v in (a, b, out)]
        rc = lib.mvba_align_robust(n, p[0], p[1], None, 1, thr, H, 1, n_refit, p[2], None, None, None, None, None, None, None, None, -1)
        return rc, lib.mvba_last_error().decode()

    for kw, text in (({"thr": 0.0}, "threshold = 0.0"), ({"thr": float("nan")}, "threshold = nan"), ({"thr": -0.5}, "threshold = -0.5"),
                     ({"H": 0}, "n_hypotheses = 0"), ({"H": 65537}, "n_hypotheses = 65537"), ({"n_refit": -1}, "n_refit = -1"),
                     ({"n_refit": 17}, "n_refit = 17"), ({"n": -1}, "n = -1"), ({"n": 1 << 31}, "n = 2147483648"),
                     ({"a": None}, "null argument: src (argument 2)"), ({"b": None}, "null argument: dst (argument 3)"),
                     ({"out": None}, "null argument: sim13 (argument 10)")):
        rc, msg = call(**kw)
        assert rc == _mvba.MVBA_ERR_BADARG and text in msg, (kw, msg)
    rc = lib.mvba_align(80, _mvba._ptr(src), _mvba._ptr(dst), None, 1, None, None, None, None, -1)
    assert rc == _mvba.MVBA_ERR_BADARG and "null argument: sim13 (argument 6)" in lib.mvba_last_error().decode()
    rc = lib.mvba_align(-3, _mvba._ptr(src), _mvba._ptr(dst), None, 1, _mvba._ptr(sim), None, None, None, -1)
    assert rc == _mvba.MVBA_ERR_BADARG and "n = -3" in lib.mvba_last_error().decode()


def test_alignment_fails_loudly_without_gpu():
    if os.path.exists(_mvba.LIB_PATH) and _mvba.device_count() > 0:
        pytest.skip("a device is visible")
    src, dst = AC.case("a80")[:2]
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        _mvba.align_robust(src, dst, 0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        _mvba.align(src, dst)


def _premises(a, b, what):
    """(a) the two routes give one count table and one of every other integer; (b) no test within GUARD of its threshold;
    (c) no sample within a factor 100 of the degeneracy rule."""
    for key in ("hyp_count", "inlier"):
        np.testing.assert_array_equal(a[key], b[key])
    for key in ("status", "best", "n_inliers", "n_usable", "n_accepted", "end"):
        assert a[key] == b[key], key
    guard = min(a["margin"], b["margin"])
    piv = a["pivot"][np.isfinite(a["pivot"])]
    near = (piv > 1e-14) & (piv < 1e-10)
    print(f"{what}: guard {guard:.2e}, sample pivots in {piv.min() if len(piv) else np.nan:.2e} .. {piv.max() if len(piv) else np.nan:.2e}")
    assert guard >= AC.GUARD and not near.any()


def _host_diff(a, b, name):
    d = np.abs(a["sim13"] - b["sim13"]).max()
    rms = abs(a["quality"][0] - b["quality"][0])
    rel = (np.abs(a["quality"][1:] - b["quality"][1:]) / np.abs(a["quality"][1:])).max()
    print(f"{name}: horn vs svd max |d(s, Q, tau)| = {d:.3e} (recorded {AC.HOST_DIFF[name]:.1e}), RMS {rms:.3e} (margin {AC.rms_margin(name):.1e}), "
          f"gap and spread relative {rel:.3e}")
    assert 0.5 * AC.HOST_DIFF[name] <= d <= AC.HOST_DIFF[name]
    assert rms <= AC.rms_margin(name) and rel <= AC.MARGIN * AC.HOST_DIFF[name]
    s, Q, _ = AR.decompose(a["sim13"])
    assert s > 0 and abs(np.linalg.det(Q) - 1.0) <= 1e-14 and np.abs(Q @ Q.T - np.eye(3)).max() <= 1e-14


@pytest.mark.parametrize("name", sorted(AC.PARITY))
def test_parity_premises_and_host_versus_host_difference(name):
    a, b = AC.reference(name), AC.reference(name, "svd")
    _premises(a, b, name)
    assert a["status"] == 0
    _host_diff(a, b, name)
    _premises(AC.reference(name, "horn", 0), AC.reference(name, "svd", 0), name + ", n_refit = 0")
    pa, pb = AC.plain_reference(name), AC.plain_reference(name, "svd")
    d = np.abs(pa["sim13"] - pb["sim13"]).max()
    print(f"{name}: plain fit of the clean rows, horn vs svd {d:.3e}")
    assert pa["status"] == 0 and d <= AC.HOST_DIFF[name]


@pytest.mark.parametrize("name", sorted(AC.PARITY))
def test_reference_recovers_exactly_the_clean_rows(name):
    """The final inliers are exactly the usable rows that were not replaced -- no replaced row lands within the threshold by chance
    on these cases (a uniform position in dst's box hits a ball of radius 0.01 s with probability 5e-7) --, the refit IS the
    least-squares fit of the clean rows, and the plain fit of all usable rows is far off."""
    src, dst, ok, ws, thr, H, seed, clean = AC.case(name)
    a, plain = AC.reference(name), AC.plain_reference(name)
    assert a["n_inliers"] == AC.N_CLEAN[name] == clean.sum() and a["n_usable"] == AR.usable(src, dst, ok).sum()
    np.testing.assert_array_equal(a["inlier"], clean)
    np.testing.assert_array_equal(a["sim13"], plain["sim13"])
    truth = AC.truth(AC.PARITY[name][1])
    err, off = np.abs(plain["sim13"] - truth).max(), np.abs(AR.align(src, dst, ok, ws)["sim13"] - plain["sim13"]).max()
    print(f"{name}: the clean fit is {err:.2e} from the truth, the plain fit of all usable rows {off:.2e} from the clean fit")
    assert err <= 1e-3 and off >= 100.0 * err
    if not ws:
        assert a["sim13"][0] == 1.0


def test_limit_premises_and_host_versus_host_differences():
    """Every structural-limit case of test_gpu_align.py: statuses, premises, recorded figures."""
    src, dst, _, ws, thr, _, seed, clean = AC.case("a80")
    for H in AC.LIMIT_H:
        a, b = AC.reference("a80", n_hyp=H), AC.reference("a80", "svd", n_hyp=H)
        _premises(a, b, f"H = {H}")
        if H == 1:
            # one hypothesis alone: sample 0 holds a replaced row, and a similarity through three rows that no similarity relates
            # passes through none of them -- its count is 0: status 4 from data
            assert a["status"] == 4 and a["best"] == 0 and a["hyp_count"][0] == 0 and not clean[AR.sample(seed, 0, 80)].all()
            continue
        assert a["status"] == 0
        _host_diff(a, b, f"h{H}")
    # exactly three usable rows: every hypothesis is a permutation of them, all counts are 3, the refit is their own fit
    src, dst, ok = AC.few_case(3)
    a, b = (AR.align_robust(src, dst, thr, ok, True, 64, 1, 2, r) for r in AR.ROUTES)
    _premises(a, b, "three")
    assert a["status"] == 0 and (a["hyp_count"] == 3).all() and a["best"] == 0 and a["n_inliers"] == 3 and a["n_usable"] == 3
    _host_diff(a, b, "three")
    src, dst, ok = AC.few_case(2)
    a = AR.align_robust(src, dst, thr, ok, True, 64, 1, 2)
    assert a["status"] == 1 and (a["hyp_count"] == -1).all() and a["n_usable"] == 2
    # src on a line, exactly: every hypothesis degenerate; the plain fit refuses it by the eigenvalue gap
    src, dst = AC.collinear_case()
    a = AR.align_robust(src, dst, thr, None, True, 64, 1, 2)
    assert a["status"] == 2 and (a["hyp_count"] == -1).all() and a["best"] == -1 and (a["pivot"] == 0.0).all()
    assert AR.align(src, dst)["status"] == 2 and AR.align(dst, src)["status"] == 2
    for n in AC.SCAN_SIZES:
        a, b = AC.scan_reference(n), AC.scan_reference(n, "svd")
        _premises(a, b, f"scan {n}")
        assert a["status"] == 0
        _host_diff(a, b, f"scan{n}")
    # the refits at a tighter threshold: the inlier set moves
    worst = 0.0
    for r in AC.REFIT_COUNTS:
        a, b = AC.refit_reference(r), AC.refit_reference(r, "svd")
        _premises(a, b, f"refits, n_refit = {r}")
        worst = max(worst, np.abs(a["sim13"] - b["sim13"]).max())
    a = AC.refit_reference(16)
    print("refits at 16:", a["n_accepted"], a["end"], a["n_inliers"], "after none:", AC.refit_reference(0)["n_inliers"], f"host figure {worst:.3e}")
    assert a["n_inliers"] != AC.refit_reference(0)["n_inliers"] and 0.5 * AC.HOST_DIFF["refits"] <= worst <= AC.HOST_DIFF["refits"]
    # H = 65 536: the sampled entries of the count table
    hs, c, guard, pivot = AC.max_hyp_reference()
    c2, guard2 = AC.max_hyp_reference("svd")[1:3]
    np.testing.assert_array_equal(c, c2)
    print(f"max hyp: guard {min(guard, guard2):.2e}, degenerate {int((c < 0).sum())} of {len(hs)}")
    assert min(guard, guard2) >= AC.GUARD and len(hs) == 739 and not ((pivot > 1e-14) & (pivot < 1e-10)).any()


def test_transform_composed_with_its_inverse_is_the_identity():
    sc = make_scene(60, 5, vis_p=0.6, project="numpy")
    sim = AC.truth(AC.SCALE)
    s, Q, tau = AR.decompose(sim)
    X, R, t = transform_reconstruction(s, Q, tau, sc.X_gt, sc.R_gt, sc.t_gt)
    for got, want in zip((X, R, t), AR.transform(sim, sc.X_gt, sc.R_gt, sc.t_gt)):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
    si, Qi, ti = AR.decompose(AR.inverse(sim))
    Xb, Rb, tb = transform_reconstruction(si, Qi, ti, X, R, t)
    d = max(np.abs(Xb - sc.X_gt).max(), np.abs(Rb - sc.R_gt).max(), np.abs(tb - sc.t_gt).max())
    print(f"similarity then its inverse: {d:.2e} from the identity")
    assert d <= 1e-12
    assert transform_reconstruction(s, Q, tau, X=sc.X_gt)[1:] == (None, None)


def test_transform_leaves_reprojections_unchanged_and_nan_rows_nan():
    sc = make_scene(60, 5, vis_p=0.6, project="numpy")
    s, Q, tau = AR.decompose(AC.truth(AC.SCALE))
    X0, R0, t0 = sc.X_gt.copy(), sc.R_gt.copy(), sc.t_gt.copy()
    X0[[3, 40]] = np.nan
    R0[2], t0[2] = np.nan, np.nan
    X, R, t = transform_reconstruction(s, Q, tau, X0, R0, t0)
    assert np.isnan(X[[3, 40]]).all() and np.isnan(R[2]).all() and np.isnan(t[2]).all()
    assert np.isfinite(np.delete(X, [3, 40], axis=0)).all() and np.isfinite(np.delete(R, 2, axis=0)).all()
    Xf, Rf, tf = transform_reconstruction(s, Q, tau, sc.X_gt, sc.R_gt, sc.t_gt)
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    f, u = sc.K_gt[:, 0, 0], sc.K_gt[:, :2, 2]
    before, after = project_obs(sc.X_gt, f, u, sc.t_gt, sc.R_gt, 1.0, pt, sc.cam_idx), project_obs(Xf, f, u, tf, Rf, 1.0, pt, sc.cam_idx)
    d = np.abs(after - before).max()
    print(f"reprojections under a similarity of points and cameras move by {d:.2e}")
    assert d <= 1e-12
