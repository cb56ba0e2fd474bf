"""mvba_pose_robust and mvba_pose_refine at their structural limits, and the camera tile loop they share with mvba_resect_robust
("Structural limits"; §18 for the DLT tile case): a second tile whose chunk offset is not its list position; the
endings of k_pose_step (the last permitted step accepted, n_refine 0 / 1 / 16, the pivot rule at the first step, three
observations); refit loops whose cameras leave RS_ACTIVE at different refits, keep a fixed point for 16 refits, keep a refit
that leaves the set as it is; k_pose_fit under sparse masks over 20 chunks; a full 3 x 3 K.  Integer outputs EXACTLY the NumPy
restatement's (tests/test_pose_ransac_cpu.py asserts the premises, and each case's structural premise, on the reference alone),
R, t and the RMS within 100 x the host-versus-host figure of the very case (tests/_pose_ransac_cases.py)."""
import numpy as np
import pytest

import _pose_ransac_cases as PC
import _pose_ransac_ref as PR
import _resect_ransac_cases as QC
from lib import _mvba

pytestmark = pytest.mark.gpu

KEYS = ("R", "t", "quality", "n_usable", "n_inliers", "best", "status", "hyp_count")
DLT_KEYS = ("P", "quality", "n_usable", "n_inliers", "best", "status", "hyp_count")
REFINE_KEYS = ("R", "t", "quality", "n_usable", "status")


def _run(X, pt_ptr, cam, xy, K, thr, H, seed, n_refine=5, n_refit=2, **kw):
    return _mvba.pose_robust(X, pt_ptr, cam, xy, K, thr, n_hypotheses=H, seed=seed, n_refine=n_refine, n_refit=n_refit, return_counts=True, **kw)


def _assert_exact(got, want, other, what):
    firm = ~PC.fragile(want, other)
    np.testing.assert_array_equal(got["hyp_count"][firm], want["hyp_count"][firm], err_msg=f"{what}: hyp_count")
    for key in ("best", "n_usable", "n_inliers", "status", "inlier"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")


def _assert_close(got, want, margin, what):
    """R, t and the RMS of the cameras of status 0 within ``margin``; returns the largest |d(R, t)|."""
    ok = want["status"] == 0
    assert ok.all()
    d = max(np.abs(got["R"] - want["R"]).max(), np.abs(got["t"] - want["t"]).max())
    dq = np.abs(got["quality"][:, 0] - want["quality"][:, 0]).max()
    print(f"{what}: max |d(R, t)| {d:.3e}, RMS {dq:.3e} (margin {margin:.1e})")
    assert d <= margin and dq <= margin
    return d


def _same_entries(a, rows_a, b, rows_b, keys, what):
    """The list entries ``rows_a`` of call a are bitwise the entries ``rows_b`` of call b, in every per-camera output."""
    for key in keys:
        x, y = np.ascontiguousarray(a[key][rows_a]), np.ascontiguousarray(b[key][rows_b])
        assert x.tobytes() == y.tobytes(), f"{what}: {key}"


def _tile_asserts(got, single, cameras, keys, cam, what):
    """Every entry of the tiled call is bitwise the single-camera call of its camera; best is the arg-max of the returned table
    (np.argmax: the lowest h on ties); the inlier bytes are the union of the single calls'."""
    for i, k in enumerate(cameras):
        _same_entries(got, slice(i, i + 1), single[k], slice(None), keys, f"{what}: entry {i} (camera {k}) and the camera alone")
    np.testing.assert_array_equal(got["best"], np.argmax(got["hyp_count"], axis=1), err_msg=what)
    union = np.zeros(len(cam), bool)
    for k in set(cameras):
        assert (cam[single[k]["inlier"]] == k).all() and single[k]["inlier"].sum() == single[k]["n_inliers"][0]
        union |= single[k]["inlier"]
    np.testing.assert_array_equal(got["inlier"], union, err_msg=what)


def test_two_tiles_of_the_pose():
    """"tiles_edges": cameras of 2, 1 and 1 chunks listed four times at H = 65 536; the tile is 10 entries, and the second starts
    at entry 10 whose first chunk is 14."""
    X, pt_ptr, cam, xy, K, thr, _, seed, _ = PC.case("edges_h65")
    cams, H = list(PC.TILE_CAMERAS), PC.TILE_HYP
    assert PC.camera_tile(len(cams), H) == 10 and PC.list_chunks(cams, np.bincount(cam))[10] == 14
    got = _run(X, pt_ptr, cam, xy, K, thr, H, seed, cameras=cams)
    single = {k: _run(X, pt_ptr, cam, xy, K, thr, H, seed, cameras=[k]) for k in range(3)}
    assert (got["status"] == 0).all()
    _tile_asserts(got, single, cams, KEYS, cam, "pose")
    want, other = PC.reference("edges_h65"), PC.other(PC.reference, "edges_h65")
    firm = ~PC.fragile(want, other)
    for i, k in enumerate(cams):  # a hypothesis depends on (seed, camera, h) alone
        np.testing.assert_array_equal(got["hyp_count"][i][:65][firm[k]], want["hyp_count"][k][firm[k]], err_msg=f"entry {i}")


def test_two_tiles_of_the_dlt():
    """The same list seven times through mvba_resect_robust at H = 65 536 (the issue's first choice; 21 x 1024 blocks of
    k_resect_hyp and the three single-camera calls): the tile is 20 entries, entry 20 starts at chunk 27."""
    X, pt_ptr, cam, xy, m, thr, _, seed, _, _ = QC.case("edges_h65")
    cams, H = list(QC.TILE_CAMERAS), QC.TILE_HYP
    assert QC.camera_tile(len(cams), H) == 20 and QC.list_chunks(cams, np.bincount(cam))[20] == 27

    def run(cameras):
        return _mvba.resect_robust(X, pt_ptr, cam, xy, m, thr, cameras=cameras, n_hypotheses=H, seed=seed, n_refit=2, return_counts=True)

    got = run(cams)
    single = {k: run([k]) for k in range(3)}
    assert (got["status"] == 0).all()
    _tile_asserts(got, single, cams, DLT_KEYS, cam, "DLT")
    want = QC.reference("edges_h65")
    for i, k in enumerate(cams):
        np.testing.assert_array_equal(got["hyp_count"][i][:65], want["hyp_count"][k], err_msg=f"entry {i}")


@pytest.mark.parametrize("name", PC.TRACE_NAMES)
def test_refit_traces_and_cameras_alone(name):
    """n_refit = 0, 1, 2, 3, 16 against the reference at the same n_refit and n_refine; a camera of the three-camera call is
    bitwise the camera called alone (its neighbours leave the loop at other refits: no state leaks inside a tile)."""
    X, pt_ptr, cam, xy, K, thr, H, seed, n_refine, _ = PC.limit_case(name)
    worst, runs = 0.0, {}
    for r in PC.LIMIT_REFIT_COUNTS:
        got, want = _run(X, pt_ptr, cam, xy, K, thr, H, seed, n_refine, r), PC.limit_reference(name, n_refit=r)
        _assert_exact(got, want, PC.other(PC.limit_reference, name, n_refit=r), f"{name}, n_refit = {r}")
        d = _assert_close(got, want, PC.limit_margin(name, r), f"{name}, n_refit = {r}")
        worst, runs[r] = max(worst, d if r else 0.0), got
        if r == 0:
            np.testing.assert_array_equal(got["n_inliers"], want["hyp_count"].max(axis=1))
    print(f"{name}: largest |d(R, t)| with refits {worst:.3e} (margin {PC.limit_margin(name, 16):.1e})")
    if n_refine == 0:  # a refit without a step keeps the pose and the set; no pivot is ever recorded
        for r in PC.LIMIT_REFIT_COUNTS:
            _same_entries(runs[r], slice(None), runs[0], slice(None), ("R", "t", "n_inliers", "inlier"), f"{name}: n_refit = {r} and 0")
            assert (runs[r]["quality"][:, 1] == 0).all()
    for k in range(3):
        one = _run(X, pt_ptr, cam, xy, K, thr, H, seed, n_refine, 16, cameras=[k])
        _same_entries(runs[16], slice(k, k + 1), one, slice(None), KEYS, f"{name}: camera {k} in the call and alone")
        np.testing.assert_array_equal(one["inlier"], runs[16]["inlier"] & (cam == k))


def test_general_K():
    """K' = 2.5 K Rod(Q): all nine cofactors of pose_bearing's adjugate, K'[2][2] != 1 in pose_matrix and pose_pass.  The camera
    matrices are those of "300x8" (up to scale), so the integers are, and R' = R Q."""
    name = "general_K"
    X, pt_ptr, cam, xy, K, thr, H, seed, n_refine, n_refit = PC.limit_case(name)
    assert (np.abs(np.asarray(K)) > 1e-3).all() and (np.abs(np.asarray(K)[:, 2, 2] - 1.0) > 0.1).all()
    got, want = _run(X, pt_ptr, cam, xy, K, thr, H, seed, n_refine, n_refit), PC.limit_reference(name)
    _assert_exact(got, want, PC.other(PC.limit_reference, name), name)
    _assert_close(got, want, PC.limit_margin(name, n_refit), name)
    plain, Q = _run(*PC.case("300x8")[:8]), PR.rodrigues(np.array(PC.Q_AXIS))
    for key in ("best", "n_usable", "n_inliers", "status", "inlier"):
        np.testing.assert_array_equal(got[key], plain[key], err_msg=key)
    firm = ~PC.fragile(want, PC.other(PC.limit_reference, name)) & ~PC.fragile(PC.reference("300x8"), PC.other(PC.reference, "300x8"))
    np.testing.assert_array_equal(got["hyp_count"][firm], plain["hyp_count"][firm])
    d = max(np.abs(got["R"] - plain["R"] @ Q).max(), np.abs(got["t"] - plain["t"]).max())
    print(f"general_K against the plain K on the device: max |R' - R Q|, |t' - t| = {d:.3e}")
    # (device' to reference', reference' to reference x Q as test_pose_ransac_cpu.py measures it, reference to device)
    assert d <= PC.limit_margin(name, n_refit) + max(PC.GENERAL_K_T_DIFF, PC.GENERAL_K_R_DIFF) + PC.MARGIN * PC.POSE_HOST_DIFF["300x8"]


def _refine(name, cameras=None):
    X, pt_ptr, cam, xy, K, R0, t0, ok, obs_ok, n_steps = PC.refine_limit_case(name)
    R0, t0, K = np.asarray(R0), np.asarray(t0), np.asarray(K)
    if cameras is not None:
        R0, t0 = R0[cameras], t0[cameras]
    return _mvba.pose_refine(X, pt_ptr, cam, xy, K, R0, t0, point_ok=ok, obs_ok=obs_ok, cameras=cameras, n_steps=n_steps)


def _refine_parity(name):
    got, (Rw, tw, qw, nw, sw, _) = _refine(name), PC.refine_limit_reference(name)
    np.testing.assert_array_equal(got["status"], sw, err_msg=name)
    np.testing.assert_array_equal(got["n_usable"], nw, err_msg=name)
    ok, margin = sw == 0, PC.MARGIN * PC.REFINE_LIMIT_HOST_DIFF[name]
    d = max(np.abs(got["R"][ok] - Rw[ok]).max(), np.abs(got["t"][ok] - tw[ok]).max())
    dq = np.abs(got["quality"][ok, :2] - qw[ok, :2]).max()
    print(f"refine {name}: max |d(R, t)| {d:.3e}, RMS {dq:.3e} (margin {margin:.1e}), steps {got['quality'][:, 2].tolist()}")
    assert d <= margin and dq <= margin
    assert (got["quality"][ok, 1] <= got["quality"][ok, 0]).all()
    return got, qw


@pytest.mark.parametrize("n_steps", PC.REFINE_STEP_COUNTS)
def test_refine_step_counts(n_steps):
    """n_steps = 1 and 2: every camera takes exactly that many steps -- the last permitted step is accepted (j == n_steps after
    an accepted pass); at 64 the iteration stops by its own rule."""
    got, qw = _refine_parity(f"steps_{n_steps}")
    if n_steps <= 2:
        np.testing.assert_array_equal(got["quality"][:, 2], np.full(8, float(n_steps)))
        np.testing.assert_array_equal(qw[:, 2], got["quality"][:, 2])
    else:
        assert (got["quality"][:, 2] >= 2).all() and (got["quality"][:, 2] < 16).all()


@pytest.mark.parametrize("name", ["masks", "masks_point_ok"])
def test_refine_under_sparse_masks(name):
    """obs_ok by 256-chunk of each camera's run over 20 chunks: full chunks, chunks without a byte set, lane 255 alone, a seeded
    half, the last chunk partial; then point_ok dropping 30 % of the points on top."""
    got, _ = _refine_parity(name)
    assert got["n_usable"].tolist() == PC.MASK_USABLE[name]
    one = _refine(name, cameras=[1])
    _same_entries(got, slice(1, 2), one, slice(None), REFINE_KEYS, f"{name}: camera 1 in the call and alone")


def test_refine_general_K():
    _refine_parity("general_K")


@pytest.mark.parametrize("name", ["statuses_a", "statuses_b"])
def test_refine_statuses_side_by_side(name):
    """Status 0 next to the pivot rule at the first step (40 collinear points; three collinear points), and the minimum of three
    observations next to two: a camera of status != 0 keeps its input pose bitwise and has NaN quality, a camera of status 0 is
    bitwise what it is when called alone."""
    R0, t0 = (np.ascontiguousarray(a) for a in PC.refine_limit_case(name)[5:7])
    got, (_, _, _, nw, sw, _) = _refine(name), PC.refine_limit_reference(name)
    assert sw.tolist() == PC.STATUS_WANT[name]
    np.testing.assert_array_equal(got["status"], sw)
    np.testing.assert_array_equal(got["n_usable"], nw)
    for k in range(3):
        if sw[k] != 0:
            assert got["R"][k].tobytes() == R0[k].tobytes() and got["t"][k].tobytes() == t0[k].tobytes() and np.isnan(got["quality"][k]).all()
        else:
            one = _refine(name, cameras=[k])
            assert one["status"][0] == 0 and np.isfinite(one["quality"][0]).all()
            _same_entries(got, slice(k, k + 1), one, slice(None), REFINE_KEYS, f"{name}: camera {k} in the call and alone")


def test_refine_with_unobserved_cameras():
    """Status 1 with n_usable 0 between active cameras: the others are bitwise the 8-camera call."""
    got, _ = _refine_parity("empty")
    X, pt_ptr, cam, xy, K, R0, t0 = PC.refine_case()
    full = _mvba.pose_refine(X, pt_ptr, cam, xy, K, R0, t0, n_steps=PC.REFINE_STEPS)
    kept = np.nonzero(got["status"] == 0)[0]
    empty = np.nonzero(got["status"] == 1)[0]
    assert empty.tolist() == [1, 4, 10] and (got["n_usable"][empty] == 0).all() and np.isnan(got["quality"][empty]).all()
    _same_entries(got, kept, full, slice(None), REFINE_KEYS, "the observed cameras among unobserved ones and alone")
    R0e, t0e = PC.refine_limit_case("empty")[5:7]
    assert got["R"][empty].tobytes() == np.ascontiguousarray(R0e[empty]).tobytes()
    assert got["t"][empty].tobytes() == np.ascontiguousarray(t0e[empty]).tobytes()
