"""Scenes shared by test_homography_cpu.py and test_gpu_homography.py, each built once, and the host-versus-host differences
(closed-form hypotheses and eigh refits against the SVD of the stacked rows) that set the parity margins -- the rule of
tests/_ransac_cases.py.  Test infrastructure only.

The planar scene is the one of the issue: make_scene(n, m, vis_p=1.0, noise=0.0) with one coordinate of every point zeroed,
projected exactly, Gaussian noise 1e-3 added.  With X[:, 0] = 0 camera 0 of the 3-camera set looks along the plane (10 degrees
above it): a pixel of noise there is five in the other image, the homography of pairs (0, 1) and (0, 2) keeps 72 .. 75 of 80 clean
points at threshold 0.01, and pair (1, 2) keeps all 80.  Pair (1, 2) is therefore the contaminated one."""
import functools

import numpy as np

import _homography_ref as HR
import _init_cases as IC
import _ransac_cases as RC
import _resect_ransac_cases as QC
import _twoview_cases as C
import _twoview_ref as T
from lib.synthetic import make_scene

MARGIN = C.MARGIN
THRESHOLD = RC.THRESHOLD
NOISE = 1e-3
# The smallest guard (tests/_homography_ref.py: inlier_test) a case may have for its integer outputs to be compared exactly.  A
# comparison a <= thr^2 w^2 differs between the device (fused multiply-adds) and NumPy by the rounding of u - x w relative to
# thr w: a few eps |x| / thr = 4e-16 x 200 (units of 1, threshold 0.01; the same ratio in pixels), squared-distance relative
# 2e-13 -- and by the hypothesis's own matrix, which the two routes of the reference compute differently too: they must agree on
# every integer (premise (a)).  1e-7 is the bound the other RANSAC tests hold, five orders above the first figure.
GUARD = 1e-7
PIXEL_F0, PIXEL_U = 512.0, np.array([320.0, 240.0])

# Host-versus-host max-abs difference of the final H (|H| = 1) over the pairs of status 0, measured by test_homography_cpu.py on
# the very cases below.  A GPU parity assert gets MARGIN x its case's figure; the RMS the same margin relative to its size.
HOST_DIFF = {"planar80x3": 2.1e-14, "planar257x2": 5.6e-15, "pixels": 2.4e-15, "noise_free": 4.2e-15, "four": 2.3e-13, "mixed": 8.6e-15,
             "h1": 6.2e-13, "h64": 8.6e-15, "h65": 8.6e-15, "refits": 1.4e-14}
# name: (n, m, zeroed coordinate, contaminated pair (k, l): image l, n_hypotheses, seed)
PARITY = {"planar80x3": (80, 3, 0, (1, 2), 512, 2), "planar257x2": (257, 2, 2, (0, 1), 64, 1), "pixels": (80, 3, 0, (1, 2), 512, 2)}
# Measured by test_homography_cpu.py (the reference, threshold 0.01, the case's own hypotheses and seed): n_inliers_H / n_inliers_F of
# every pair "auto" is asked about.  The planar pairs, contaminated or not, against the general scenes' pair (0, 1).
RATIO_PLANAR = {("planar80x3", (0, 1)): 0.9000, ("planar80x3", (1, 2)): 0.9032, ("planar257x2", (0, 1)): 0.9072, ("pixels", (1, 2)): 0.9032}
RATIO_GENERAL = {"300x8": 0.1786, "2000x3": 0.0170}
# The contaminated grazing pair ("planar80x3", (0, 2)): 0.7576 -- H keeps 50 of 56 clean points, F adds 10 replaced ones that lie near
# their epipolar lines by chance.  It is BELOW planar_ratio = 0.8: "auto" takes the fundamental matrix there and the pose is
# wrong.  Recorded as a limit of the rule, not hidden.
RATIO_GRAZING = 0.7576
# relative_pose on the contaminated pair (1, 2) of "planar80x3": max-abs error over R_l and t_l of the reference's homography pose,
# of the 8-point pose of the UNcontaminated pair, and the host-versus-host difference of the former
POSE_H_ERR, POSE_F8_ERR, POSE_HOST_DIFF = 1.62e-2, 7.6e-1, 5.8e-15
POSE_FACTOR = 20.0  # the homography pose is closer to the truth than the uncontaminated 8-point pose by at least this factor


@functools.lru_cache(maxsize=None)
def planar_scene(n, m, axis, vis_p=1.0, noise_seed=3):
    """(scene, X on the plane, noisy xy)."""
    sc = make_scene(n, m, vis_p=vis_p, noise=0.0, project="numpy")
    X = sc.X_gt.copy()
    X[:, axis] = 0.0
    xy = IC.exact_xy(sc, X) + np.random.default_rng(noise_seed).normal(0.0, NOISE, (sc.n_obs, 2))
    for a in (X, xy):
        a.setflags(write=False)
    return sc, X, xy


@functools.lru_cache(maxsize=None)
def case(name):
    """(pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses, seed, bad, K) of a parity case: every pair k < l and the
    contaminated pair reversed; ``bad`` is over the contaminated pair's shared list; ``K`` (m, 3, 3) projects to the units of xy."""
    n, m, axis, cp, H, seed = PARITY[name]
    sc, _, xy = planar_scene(n, m, axis)
    xy, bad = RC.contaminate(sc.pt_ptr, sc.cam_idx, xy, cp[0], cp[1], 0.3)
    K, thr = sc.K_gt.copy(), THRESHOLD
    if name == "pixels":
        xy, thr = PIXEL_F0 * xy + PIXEL_U, THRESHOLD * PIXEL_F0
        K[:, 0, 0] = K[:, 1, 1] = PIXEL_F0
        K[:, :2, 2] = PIXEL_U
    pairs = np.concatenate([C.all_pairs(m), np.array([cp[::-1]], np.int32)])
    for a in (xy, bad, K):
        a.setflags(write=False)
    return sc.pt_ptr, sc.cam_idx, xy, m, pairs, thr, H, seed, bad, K


@functools.lru_cache(maxsize=None)
def reference(name, route="closed", n_refit=2, n_hyp=None, **alter):
    pt_ptr, cam, xy, m, pairs, thr, H, seed, _, _ = case(name)
    return HR.homography_robust(pt_ptr, cam, xy, m, pairs, thr, H if n_hyp is None else n_hyp, seed, n_refit, route, **alter)


def true_pose(name, k, l):
    n, m, axis = PARITY[name][:3]
    return C.true_relative_pose(planar_scene(n, m, axis)[0], k, l)


def pose_error(R, t, Rg, tg):
    return max(np.abs(R[1] - Rg).max(), np.abs(t[1] - tg).max())


@functools.lru_cache(maxsize=None)
def reference_pose(name="planar80x3", model="homography", route="closed"):
    pt_ptr, cam, xy, m, _, thr, H, seed, _, K = case(name)
    return HR.relative_pose(pt_ptr, cam, xy, K, PARITY[name][3], thr, model, n_hyp=H, seed=seed, route=route)


@functools.lru_cache(maxsize=None)
def general_pose(name):
    """The reference's relative_pose(model="auto") on pair (0, 1) of a general scene of tests/_ransac_cases.py."""
    pt_ptr, cam, xy, m, _, thr, H, seed, _ = RC.case(name)
    return HR.relative_pose(pt_ptr, cam, xy, np.tile(np.eye(3), (m, 1, 1)), (0, 1), thr, "auto", n_hyp=H, seed=seed)


@functools.lru_cache(maxsize=None)
def noise_free_case():
    """tests/_twoview_cases.py's noise-free planar pair (status 2 for the fundamental matrix), both ways round."""
    pt_ptr, cam, xy, m, pair = C.degenerate_case("planar")
    return pt_ptr, cam, xy, m, np.array([pair, pair[::-1]], np.int32)


# ---- structural limits ----
COLLINEAR_CAMERA, FEW_CAMERA = 4, 3


@functools.lru_cache(maxsize=None)
def mixed_case():
    """"planar80x3" with two more cameras: camera 3 sees points 0, 1, 2 alone (status 1 WITH shared points), camera 4 sees every
    point on the line y = x / 2 + 1 / 4 at x = (j - 40) / 64 (exact in binary: every determinant is 0, status 2).
    (pt_ptr, cam_idx, xy, 5, pairs, expected status)."""
    pt_ptr, cam, xy, m, _, thr, H, seed, _, _ = case("planar80x3")
    xy3 = np.asarray(xy).reshape(80, 3, 2)
    cams, zs = [], []
    for j in range(80):
        c = [0, 1, 2] + ([FEW_CAMERA] if j < 3 else []) + [COLLINEAR_CAMERA]
        x = (j - 40) / 64.0
        z = [xy3[j, 0], xy3[j, 1], xy3[j, 2]] + ([xy3[j, 1]] if j < 3 else []) + [np.array([x, 0.5 * x + 0.25])]
        cams.append(c)
        zs.append(z)
    ptr = np.concatenate([[0], np.cumsum([len(c) for c in cams])]).astype(np.int64)
    pairs = np.array([(0, 1), (0, 3), (4, 0), (1, 2), (3, 4), (2, 1), (1, 4), (0, 2), (3, 1)], np.int32)
    want = np.array([0, 1, 2, 0, 1, 0, 2, 0, 1], np.int32)
    out_xy = np.concatenate([np.stack(z) for z in zs])
    out_xy.setflags(write=False)
    return ptr, np.concatenate(cams).astype(np.int32), out_xy, 5, pairs, want


@functools.lru_cache(maxsize=None)
def mixed_reference(route="closed"):
    ptr, cam, xy, m, pairs, _ = mixed_case()
    return HR.homography_robust(ptr, cam, xy, m, pairs, THRESHOLD, 64, 2, 2, route)


@functools.lru_cache(maxsize=None)
def few_case(n_keep):
    """The first ``n_keep`` points of "planar80x3", pair (0, 1): (pt_ptr, cam_idx, xy, 3, pairs)."""
    pt_ptr, cam, xy, m, _, _, _, _, _, _ = case("planar80x3")
    return pt_ptr[: n_keep + 1].copy(), cam[: 3 * n_keep].copy(), np.asarray(xy)[: 3 * n_keep].copy(), 3, np.array([(0, 1)], np.int32)


MAX_HYP = RC.MAX_HYP
HYP_BYTES, POINT_BYTES = 160, 48  # csrc/mvba_homography.h: HomogFit::HYP_BYTES (72 H, 72 H^-1, 4 count, rounded up); RS_POINT_BYTES


def pair_tile(n_points, n_pairs, n_hyp):
    """The number of pairs mvba_homography_robust takes per tile ("Tiles")."""
    return max(1, min(n_pairs, C.TV_MAX_TILE, C.TV_PART_BYTES // (POINT_BYTES * n_points + HYP_BYTES * n_hyp)))


def max_hyp_sample():
    return RC.max_hyp_sample()


@functools.lru_cache(maxsize=None)
def max_hyp_reference(which, route="closed"):
    """(h, counts, guard, pivot) at the h of max_hyp_sample(): "four" -- the 4-point pair -- or "eighty" -- "planar80x3" (1, 2)."""
    if which == "four":
        pt_ptr, cam, xy, m, pairs = few_case(4)
        k, l, thr, seed = 0, 1, THRESHOLD, 2
    else:
        pt_ptr, cam, xy, m, _, thr, _, seed, _, _ = case("planar80x3")
        k, l = 1, 2
    _, xk, xl = T.shared(pt_ptr, cam, np.asarray(xy).reshape(-1, 2), k, l)
    hs = max_hyp_sample()
    return (hs,) + HR.hypothesis_counts(xk, xl, k, l, thr, seed, hs, route)


REFIT_COUNTS = (0, 1, 16)
REFIT_THRESHOLD = 6e-3  # "planar80x3" at a tighter threshold: the inlier sets move and the pairs leave the loop at different refits


@functools.lru_cache(maxsize=None)
def refit_reference(n_refit, route="closed"):
    pt_ptr, cam, xy, m, pairs, _, H, seed, _, _ = case("planar80x3")
    return HR.homography_robust(pt_ptr, cam, xy, m, pairs, REFIT_THRESHOLD, H, seed, n_refit, route)


# ---- bootstrap ----
BOOT_AXIS = 0  # the coordinate zeroed in the bootstrap scene (see bootstrap_case)


@functools.lru_cache(maxsize=None)
def bootstrap_case():
    """make_scene(300, 8, vis_p=0.5) with X[:, BOOT_AXIS] = 0, noise 1e-3, and 20 % of the observations of cameras 2 .. 7 replaced as
    in tests/_resect_ransac_cases.py: (scene, X, xy', replaced)."""
    sc, X, xy = planar_scene(300, 8, BOOT_AXIS, vis_p=0.5)
    xy, hit = QC.contaminate(sc.cam_idx, xy, QC.BOOT_FRACTION, cameras=np.arange(2, 8))
    for a in (xy, hit):
        a.setflags(write=False)
    return sc, X, xy, hit


@functools.lru_cache(maxsize=None)
def reference_bootstrap(route="closed"):
    from lib.initialization import engine_intrinsics

    sc, _, xy, _ = bootstrap_case()
    return HR.bootstrap(sc.pt_ptr, sc.cam_idx, xy, engine_intrinsics(sc.init_K), THRESHOLD, THRESHOLD, "auto", 512, 1, route, start_pair=(0, 1),
                        max_rms=0.01)


@functools.lru_cache(maxsize=None)
def ambiguous_case():
    """bootstrap_case() without the shared points of pair (0, 1) that the second rotation's plane puts behind camera 0: the two
    views of the pair then allow two poses with every inlier in front of both cameras, and only a third camera can tell them
    apart.  (scene, pt_ptr, cam_idx, xy', replaced, kept point ids)."""
    from lib.initialization import engine_intrinsics

    sc, _, xy, hit = bootstrap_case()
    K = engine_intrinsics(sc.init_K)
    info = HR.homography_pose(sc.pt_ptr, sc.cam_idx, xy, K, (0, 1), THRESHOLD, 512, 1)[3]
    nf = info["n_front"]
    loser = [c for c in np.argsort(-nf, kind="stable") if info["candidates"][c][0] is not info["candidates"][int(np.argmax(nf))][0]][0]
    ids, xk, _ = T.shared(sc.pt_ptr, sc.cam_idx, np.asarray(xy), 0, 1)
    rays = np.linalg.solve(K[0], np.c_[xk, np.ones(len(xk))].T).T
    keep_pt = np.ones(sc.n_points, bool)
    side = rays @ info["candidates"][loser][2]
    keep_pt[ids[side <= 0.25 * np.median(side[side > 0])]] = False  # (well inside: the refit of the smaller set moves the plane a little)
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    keep = keep_pt[pt]
    ptr = np.concatenate([[0], np.cumsum(np.diff(sc.pt_ptr)[keep_pt])]).astype(np.int64)
    out = (sc, ptr, sc.cam_idx[keep], np.asarray(xy)[keep], hit[keep], np.nonzero(keep_pt)[0])
    for a in out[3:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ambiguous_reference(route="closed"):
    from lib.initialization import engine_intrinsics

    sc, ptr, cam, xy, _, _ = ambiguous_case()
    return HR.bootstrap(ptr, cam, xy, engine_intrinsics(sc.init_K), THRESHOLD, THRESHOLD, "auto", 512, 1, route, start_pair=(0, 1), max_rms=0.01)
