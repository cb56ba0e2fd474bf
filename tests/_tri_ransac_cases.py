"""Scenes shared by test_tri_ransac_cpu.py and test_gpu_tri_ransac.py, each built once: the shapes of tests/_init_cases.py seen
through their GROUND-TRUTH cameras, with the contamination of tests/_resect_ransac_cases.py applied to the observations of ALL
cameras, and the host-versus-host differences that set the parity margins -- the rule of tests/_init_cases.py (beside its
TRI_HOST_DIFF: the plain triangulation's figures for the same scenes).  Test infrastructure only."""
import functools

import numpy as np

import _init_cases as IC
import _resect_ransac_cases as QC
import _tri_ransac_ref as TR

MARGIN = IC.MARGIN
THRESHOLD = 0.01  # ten times the noise of the scenes
FRACTION = 0.2    # of every camera's observations replaced
SEED = 1

# name: (scene of _init_cases.tri_scene, n_hypotheses)
PARITY = {"300x8": ("300x8", 64),          # degrees 3 .. 8: at most 28 pairs, every point exhaustive
          "65x70_h64": ("65x70", 64),      # degree 70, 2415 pairs: the sampled branch
          "65x70_h1": ("65x70", 1),        # one hypothesis: lanes 1 .. 15 of a group have none
          "65x70_h17": ("65x70", 17),      # no multiple of the group width: lane 0 has two, the others one
          "dense": ("dense", 64),          # the dense grid (pt_ptr = None), degree 5
          "pixels": ("pixels", 64),        # f0 = 600: raw pixel observations, the threshold in pixels
          "300x1704": ("300x1704", 64)}    # the LDS camera table at its cap; degrees 18 .. 50: sampled but for a few points

# Host-versus-host max-abs difference over the points of status 0 -- refits by eigh of the moment matrix and rays by the adjugate
# against refits by the SVD of the stacked rows and rays by np.linalg.solve --, measured by test_tri_ransac_cpu.py on the very
# cases below: X and the three quality figures of the LINEAR refit (n_refine = 0: after two Gauss-Newton steps the two routes
# agree to 1e-15 or better, which measures the convergence, not the arithmetic; tests/_init_cases.py says the same of
# TRI_HOST_DIFF).  A GPU parity assert gets MARGIN x its case's figure, for n_refine = 0 and 2 alike.
TRI_RANSAC_HOST_DIFF = {"300x8": 1.3e-14, "65x70_h64": 6.1e-15, "65x70_h1": 1.8e-15, "65x70_h17": 6.1e-15, "dense": 1.5e-14,
                        "pixels": 1.3e-13,  # (the RMS residual, in pixels; max |dX| is 1.2e-14)
                        "300x1704": 1.5e-14}
# the same for n_refit = 0: X is the best MIDPOINT (the two routes differ in the rays alone), on "300x8" at THRESHOLD and at
# REFIT_THRESHOLD (refit_reference below)
MIDPOINT_HOST_DIFF = {"300x8": 2.0e-13, "refit": 3.0e-14}
# ... and for the status shapes (status_case below)
STATUS_HOST_DIFF = 2.8e-15


def gt_args(scene):
    """(K, R, t, pt_ptr, cam_idx, xy (n_obs, 2), threshold) of a scene through its ground-truth cameras; "pixels": K maps to raw
    pixels (K[2, 2] = 1), xy and the threshold are in pixels."""
    sc = IC.tri_scene(scene)
    K, xy, thr = sc.K_gt, sc.xy, THRESHOLD
    if scene == "pixels":
        A = np.array([[IC.PIXEL_F0, 0.0, IC.PIXEL_U[0]], [0.0, IC.PIXEL_F0, IC.PIXEL_U[1]], [0.0, 0.0, 1.0]])
        K, xy, thr = A @ sc.K_gt, IC.PIXEL_F0 * sc.xy + IC.PIXEL_U, THRESHOLD * IC.PIXEL_F0
    return K, sc.R_gt, sc.t_gt, sc.pt_ptr, sc.cam_idx, xy, thr


@functools.lru_cache(maxsize=None)
def case(name):
    """(K, R, t, pt_ptr, cam_idx, xy, threshold, n_hypotheses, replaced (n_obs,)) of a parity case as the library takes it."""
    scene, H = PARITY[name]
    K, R, t, pt_ptr, cam, xy, thr = gt_args(scene)
    xy, hit = QC.contaminate(cam, xy, FRACTION)
    if scene == "dense":
        pt_ptr, cam, xy = None, None, xy.reshape(-1, len(K), 2)
    for a in (xy, hit):
        a.setflags(write=False)
    return K, R, t, pt_ptr, cam, xy, thr, H, hit


@functools.lru_cache(maxsize=None)
def reference(name, n_refine=2, n_refit=2, linear="eigh", rays="adjugate"):
    K, R, t, pt_ptr, cam, xy, thr, H, _ = case(name)
    return TR.triangulate_robust(K, R, t, pt_ptr, cam, xy, thr, H, SEED, n_refine, n_refit, linear, rays)


REFIT_COUNTS = (0, 1, 16)
# the refit trace: "300x8" at a threshold of three times the noise, where a refit changes an inlier set
REFIT_THRESHOLD = 3e-3


@functools.lru_cache(maxsize=None)
def refit_reference(n_refit, linear="eigh", rays="adjugate"):
    K, R, t, pt_ptr, cam, xy, _, H, _ = case("300x8")
    return TR.triangulate_robust(K, R, t, pt_ptr, cam, xy, REFIT_THRESHOLD, H, SEED, 2, n_refit, linear, rays)


ALL_REPLACED, ONE_OF_THREE, TWO_VIEWS = 20, 21, 22  # points of status_case() that get a shape of their own


@functools.lru_cache(maxsize=None)
def status_case():
    """_init_cases.status_case() (noise-free; point 3 seen once, point 7 by two cameras at one centre, point 11 at infinity, the
    others by cameras 0, 1, 2) with three more shapes: every observation of point 20 replaced, one of the three of point 21
    replaced, and point 22 seen by cameras 0 and 1 only.  (K, R, t, pt_ptr, cam_idx, xy)."""
    K, R, t, pt_ptr, cam, xy, _, _ = IC.status_case()
    xy, keep = xy.copy(), np.ones(len(cam), bool)
    rng = np.random.default_rng(11)
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    o = np.arange(pt_ptr[ALL_REPLACED], pt_ptr[ALL_REPLACED + 1])
    xy[o] = lo + rng.random((len(o), 2)) * (hi - lo)
    xy[pt_ptr[ONE_OF_THREE] + 1] = lo + rng.random(2) * (hi - lo)
    keep[pt_ptr[TWO_VIEWS] + 2] = False
    deg = np.diff(pt_ptr)
    deg[TWO_VIEWS] = 2
    out = K, R, t, np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), cam[keep], xy[keep]
    for v in out:
        v.setflags(write=False)
    return out


STATUS_HYP = 16


@functools.lru_cache(maxsize=None)
def status_reference(linear="eigh", rays="adjugate"):
    return TR.triangulate_robust(*status_case(), THRESHOLD, STATUS_HYP, SEED, 2, 2, linear, rays)


def clean_sets(name):
    """(points with at least three clean observations (N,) bool, clean (n_obs,) bool) of a parity case."""
    _, _, _, pt_ptr, cam, xy, _, _, hit = case(name)
    if pt_ptr is None:
        pt_ptr, _ = IC.ref.dense_list(xy.shape[0], xy.shape[1])
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    return np.bincount(pt[~hit], minlength=len(pt_ptr) - 1) >= 3, ~hit


def max_diff(a, b):
    """(max |dX|, max |dquality| (3,)) over the points of status 0 of two results with equal statuses."""
    ok = a["status"] == 0
    if not ok.any():
        return 0.0, np.zeros(3)
    return np.abs(a["X"][ok] - b["X"][ok]).max(), np.abs(a["quality"][ok] - b["quality"][ok]).max(axis=0)


# ---- bootstrap: "300x8" with FRACTION of the observations of ALL cameras replaced, the three thresholds set ----------------
BOOT_RANSAC_THRESHOLD = 0.01  # tests/_ransac_cases.py: THRESHOLD
BOOT_HYP = 512
BOOT_DELTA = 5e-3  # the Huber scale of the BA that follows: five times the noise
# measured by test_tri_ransac_cpu.py on the reference runs: host-versus-host difference of poses and points (max abs)
BOOT_HOST_DIFF = 1.1e-11
BOOT_FAR = 0.1  # a kept point farther than this from the truth (output frame, |t_1 - t_0| = 1; the median error is 0.04) is "far"
# (points kept, far) with triangulate_threshold and (points kept, far) without, on the reference runs
BOOT_REFERENCE_FIGURES = (205, 7, 300, 88)
BOOT_CONTRAST = 5  # "measurably worse": the plain run has at least this many times the far points of the robust one


@functools.lru_cache(maxsize=None)
def bootstrap_case():
    """(scene, xy', replaced): every camera's observations contaminated, 0 and 1 included."""
    sc = IC.tri_scene("300x8")
    xy, hit = QC.contaminate(sc.cam_idx, sc.xy, FRACTION)
    for a in (xy, hit):
        a.setflags(write=False)
    return sc, xy, hit


@functools.lru_cache(maxsize=None)
def reference_bootstrap(robust=True, linear="eigh", rays="adjugate"):
    """The reference driver with ransac_threshold and resect_threshold, and with (robust) or without triangulate_threshold."""
    from lib.initialization import engine_intrinsics

    sc, xy, _ = bootstrap_case()
    return TR.bootstrap(sc.pt_ptr, sc.cam_idx, xy, engine_intrinsics(sc.init_K), BOOT_RANSAC_THRESHOLD, THRESHOLD,
                        THRESHOLD if robust else None, BOOT_HYP, SEED, start_pair=(0, 1), linear=linear, rays=rays)


def point_error(sc, X, point_ok):
    """|X - X_gt| per kept point, in bootstrap's output frame (camera 0 at the origin, |t_1 - t_0| = 1)."""
    R0, t0, s = sc.R_gt[0], sc.t_gt[0], np.linalg.norm(sc.t_gt[1] - sc.t_gt[0])
    return np.linalg.norm(X[point_ok] - (((sc.X_gt - t0) @ R0) / s)[point_ok], axis=1)
