"""Scenes shared by test_pose_ransac_cpu.py, test_gpu_pose_ransac.py and test_gpu_pose_limits.py, each built once: the shapes
of tests/_init_cases.py with the contamination of tests/_resect_ransac_cases.py and the ground-truth intrinsics, and the
host-versus-host figures (np.roots and the Cholesky step against the Ferrari factorisation and lstsq) that set the parity
margins.  Test infrastructure only."""
import functools

import numpy as np

import _init_cases as IC
import _pose_ransac_ref as PR
import _resect_ransac_cases as QC
from lib.initialization import engine_intrinsics
from lib.synthetic import make_scene

MARGIN = IC.MARGIN
THRESHOLD = QC.THRESHOLD
FRAGILE_CAP = 0.01  # of a case's count table may differ between the two root finders (a near-double root); never a best one
# Host-versus-host max-abs difference of the final R and t over the cameras of status 0 and of the RMS, measured by
# test_pose_ransac_cpu.py on the very cases below (route "roots" + "chol" against "ferrari" + "lstsq").  A GPU parity assert
# gets MARGIN x its case's figure.
POSE_HOST_DIFF = {"300x8": 1.2e-9, "5000x3": 2.2e-11, "edges_h1": 1.0e-10, "edges_h65": 1.0e-10, "dense": 1.9e-10, "pixels": 2.3e-10,
                  "900x300": 5.5e-9, "coplanar_noisy": 1.7e-10,
                  # n_refit = 0: the best minimal-sample pose itself (the two root finders after the same polish)
                  "300x8_refit0": 7.9e-14,
                  # the status shapes (STATUS_NAMES below; "collinear" has no camera of status 0)
                  "four": 2.7e-15, "empty": 3.8e-10, "point_ok": 1.1e-10, "nan_X": 1.1e-10, "all_replaced": 1.3e-9}
# Most of these are the size of the LAST Gauss-Newton step: near convergence the cost moves by rounding only, and whether the
# fifth step "does not raise the cost" can differ between two routes.
# Each case's margin: the smallest |d^2 / threshold^2 - 1| over every distance either route compared with the threshold -- the
# premise under which exact counts may be asked of the device (far above the rounding of a squared distance, about 1e-12)
POSE_MARGIN = {"300x8": 1.0e-4, "5000x3": 1.2e-4, "edges_h1": 0.36, "edges_h65": 7.2e-4, "dense": 1.1e-3, "pixels": 1.0e-4, "900x300": 2.8e-5,
               "coplanar_noisy": 7.1e-4}
# the same for the refit trace (refit_reference below), by n_refit; its margin
REFIT_HOST_DIFF, REFIT_MARGIN = {0: 9.8e-15, 1: 8.9e-16, 2: 8.8e-10, 16: 2.3e-11}, 1.1e-5
# The trace is ONE case -- one scene, one threshold, the same iteration cut at four places -- and the figure of a run with refits
# is the case's, the largest of the three: whether a last step of 1e-12 "does not raise the cost" is decided by the rounding of
# two sums of 2600 squares, and at n_refit = 1 the two host routes happen to decide alike (8.9e-16), which says nothing about a
# third summation order.  Without refits nothing is iterated: that run keeps its own figure.
REFIT_TRACE_DIFF = {r: REFIT_HOST_DIFF[0] if r == 0 else max(v for k, v in REFIT_HOST_DIFF.items() if k > 0) for r in REFIT_HOST_DIFF}
# refine_poses from the perturbed ground truth of "300x8" (refine_case below): chol against lstsq
REFINE_HOST_DIFF = 2.9e-10
# bootstrap with pose_threshold on the contaminated tracks of _resect_ransac_cases.bootstrap_case(): host-versus-host difference
# of poses and points (max abs) and the pose error against the ground truth (R, t; max abs over the registered cameras) -- the
# uncontaminated plain bootstrap has (2.71e-2, 2.32e-2), the robust DLT (3.00e-2, 2.48e-2)
BOOT_HOST_DIFF, BOOT_POSE_ERR = 2.3e-9, (1.96e-2, 2.43e-2)


# name: (resection shape of _init_cases.resect_case, fraction replaced, n_hypotheses, seed)
PARITY = {"300x8": ("300x8", 0.3, 512, 1), "5000x3": ("5000x3", 0.4, 100, 1), "edges_h1": ("edges", 0.3, 1, 1),
          "edges_h65": ("edges", 0.3, 65, 1), "dense": ("dense", 0.3, 64, 1), "pixels": ("300x8", 0.3, 512, 1), "900x300": ("900x300", 0.3, 64, 1),
          "coplanar_noisy": ("coplanar", 0.3, 64, 1)}
COPLANAR_NOISE = 1e-3


@functools.lru_cache(maxsize=None)
def true_K(shape):
    """The ground-truth intrinsics of a resection shape of _init_cases.resect_case, scaled to K[2][2] = 1: the scene rebuilt by
    the very call that made the shape."""
    if shape in ("300x8", "dense"):
        sc = IC.tri_scene(shape)
    else:
        n, m, vis, noise = {"5000x3": (5000, 3, 1.0, 1e-3), "edges": (257, 3, 1.0, 1e-3), "900x300": (900, 300, 0.06, 1e-3),
                            "coplanar": (80, 3, 1.0, 0.0), "four": (60, 4, 1.0, 0.0)}[shape]
        sc = make_scene(n, m, vis_p=vis, noise=noise, project="numpy")
    return engine_intrinsics(sc.K_gt), sc


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, pt_ptr, cam_idx, xy, K, threshold, n_hypotheses, seed, replaced) of a parity case."""
    shape, frac, H, seed = PARITY[name]
    X, pt_ptr, cam, xy, m, _ = IC.resect_case(shape)
    K, thr = true_K(shape)[0], THRESHOLD
    if name == "pixels":  # f0 = 600: raw pixel observations, the threshold in pixels
        A = np.array([[IC.PIXEL_F0, 0.0, IC.PIXEL_U[0]], [0.0, IC.PIXEL_F0, IC.PIXEL_U[1]], [0.0, 0.0, 1.0]])
        xy, thr, K = IC.pixel_scene()[1], THRESHOLD * IC.PIXEL_F0, A @ K
    if name == "coplanar_noisy":
        xy = xy + np.random.default_rng(11).normal(0.0, COPLANAR_NOISE, xy.shape)
    xy, hit = QC.contaminate(cam, xy, frac)
    if name == "dense":  # the dense grid: pt_ptr = None, xy (N, m, 2)
        pt_ptr, cam, xy = None, None, xy.reshape(len(X), m, 2)
    for a in (xy, hit, K):
        a.setflags(write=False)
    return X, pt_ptr, cam, xy, K, thr, H, seed, hit


@functools.lru_cache(maxsize=None)
def reference(name, roots="roots", solver="chol", n_refit=2):
    X, pt_ptr, cam, xy, K, thr, H, seed, _ = case(name)
    return PR.pose_robust(X, pt_ptr, cam, xy, K, thr, n_hyp=H, seed=seed, n_refit=n_refit, roots=roots, solver=solver)


def other(fn, *args, **kw):
    """The second host route of a reference function."""
    return fn(*args, roots="ferrari", solver="lstsq", **kw)


def fragile(a, b):
    """(C, H) bool: the hypotheses whose count differs between two routes."""
    return a["hyp_count"] != b["hyp_count"]


STATUS_HYP, STATUS_SEED = 16, 1
ALL_REPLACED_CAMERA = QC.ALL_REPLACED_CAMERA


@functools.lru_cache(maxsize=None)
def status_case(name):
    """(X, pt_ptr, cam_idx, xy, K, point_ok or None, expected status or None) of a status shape (n_hypotheses 16, seed 1)."""
    if name == "four":  # camera 1: exactly 4 usable observations, every hypothesis is the same set; camera 2: 3 (status 1); noise-free
        K, sc = true_K("four")
        pt = np.repeat(np.arange(60), 4)
        keep = ~(((sc.cam_idx == 1) & (pt >= 4)) | ((sc.cam_idx == 2) & (pt >= 3)))
        pt_ptr = np.concatenate([[0], np.cumsum(np.bincount(pt[keep], minlength=60))]).astype(np.int64)
        return sc.X_gt, pt_ptr, sc.cam_idx[keep], sc.xy[keep], K, None, np.array([0, 0, 1, 0], np.int32)
    if name == "collinear":  # every point on one line: no triangle has a frame
        K, sc = true_K("coplanar")
        X = sc.X_gt[0] + np.linspace(-1.0, 1.0, 80)[:, None] * np.array([0.3, 0.5, 0.2])
        return X, sc.pt_ptr, sc.cam_idx, IC.exact_xy(sc, X), K, None, np.full(3, 2, np.int32)
    if name == "empty":  # cameras 1, 4 and 10 unobserved among observed ones
        X, pt_ptr, cam, xy, m, kept = IC.empty_camera_case()
        K = np.tile(np.eye(3), (m, 1, 1))
        K[kept] = true_K("300x8")[0]
        want = np.zeros(m, np.int32)
        want[list(IC.EMPTY_CAMERAS)] = 1
        return X, pt_ptr, cam, QC.contaminate(cam, xy, 0.3)[0], K, None, want
    X, pt_ptr, cam, xy, m, _ = IC.resect_case("300x8")
    K = true_K("300x8")[0]
    if name in ("point_ok", "nan_X"):  # a seeded 70 % of the points usable: by the mask, or by NaN in X
        ok = np.random.default_rng(3).random(len(X)) < 0.7
        xy = QC.contaminate(cam, xy, 0.3)[0]
        if name == "point_ok":
            return X, pt_ptr, cam, xy, K, ok, np.zeros(m, np.int32)
        return np.where(ok[:, None], X, np.nan), pt_ptr, cam, xy, K, None, np.zeros(m, np.int32)
    if name == "all_replaced":  # every observation of camera 3 replaced, 30 % of the others'
        xy = QC.contaminate(cam, xy, 0.3)[0]
        xy = QC.contaminate(cam, xy, 2.0, seed=9, cameras=[ALL_REPLACED_CAMERA])[0]
        return X, pt_ptr, cam, xy, K, None, None  # (camera 3: whatever the reference says)
    raise KeyError(name)


STATUS_NAMES = ("four", "collinear", "empty", "point_ok", "nan_X", "all_replaced")


@functools.lru_cache(maxsize=None)
def status_reference(name, roots="roots", solver="chol"):
    X, pt_ptr, cam, xy, K, ok, _ = status_case(name)
    return PR.pose_robust(X, pt_ptr, cam, xy, K, THRESHOLD, point_ok=ok, n_hyp=STATUS_HYP, seed=STATUS_SEED, roots=roots, solver=solver)


# the refit trace: "5000x3" at a threshold of twice the noise
REFIT_THRESHOLD, REFIT_COUNTS = QC.REFIT_THRESHOLD, QC.REFIT_COUNTS


@functools.lru_cache(maxsize=None)
def refit_reference(n_refit, roots="roots", solver="chol"):
    X, pt_ptr, cam, xy, K, _, H, seed, _ = case("5000x3")
    return PR.pose_robust(X, pt_ptr, cam, xy, K, REFIT_THRESHOLD, n_hyp=H, seed=seed, n_refit=n_refit, roots=roots, solver=solver)


TV_PART_BYTES, PR_HYP_BYTES, MAX_TILE = 128 << 20, 196, 65535  # csrc/mvba_twoview.h, csrc/mvba_pose_ransac.h


def camera_tile(n_cameras, n_hyp):
    """The number of cameras mvba_pose_robust takes per tile: the documented formula restated (see
    _resect_ransac_cases.camera_tile for what that can and cannot show)."""
    return max(1, min(n_cameras, MAX_TILE, TV_PART_BYTES // (PR_HYP_BYTES * n_hyp)))


REFINE_PERTURBATION, REFINE_STEPS = 1e-2, 10


@functools.lru_cache(maxsize=None)
def refine_case():
    """The ground-truth poses of "300x8" perturbed by a seeded 1e-2 (t by normal noise, R by a rotation of that size), on the
    clean observations: (X, pt_ptr, cam_idx, xy, K, R0, t0)."""
    K, sc = true_K("300x8")
    rng = np.random.default_rng(5)
    t0 = sc.t_gt + rng.normal(0.0, REFINE_PERTURBATION, sc.t_gt.shape)
    R0 = np.stack([PR.rodrigues(w) for w in rng.normal(0.0, REFINE_PERTURBATION, (8, 3))]) @ sc.R_gt
    for a in (R0, t0):
        a.setflags(write=False)
    return sc.X_gt, sc.pt_ptr, sc.cam_idx, sc.xy, K, R0, t0


@functools.lru_cache(maxsize=None)
def refine_reference(solver="chol"):
    X, pt_ptr, cam, xy, K, R0, t0 = refine_case()
    return PR.pose_refine(X, pt_ptr, cam, xy, K, R0, t0, n_steps=REFINE_STEPS, solver=solver)


@functools.lru_cache(maxsize=None)
def reference_bootstrap(roots="roots", solver="chol"):
    sc, xy, _ = QC.bootstrap_case()
    return PR.bootstrap(sc.pt_ptr, sc.cam_idx, xy, engine_intrinsics(sc.init_K), THRESHOLD, 512, 1, start_pair=(0, 1), max_rms=0.01, roots=roots,
                        solver=solver)


# ---- The structural limits ("Structural limits"): test_gpu_pose_limits.py, premises in test_pose_ransac_cpu.py ----
LIMIT_REFIT_COUNTS = (0, 1, 2, 3, 16)  # the n_refit at which the trace cases run on the device
# name: (parity case that gives the scene, threshold, n_hypotheses, seed, n_refine, n_refit)
LIMITS = {"refits_1.2e-3": ("5000x3", 1.2e-3, 100, 1, 5, 16), "refits_2.5e-3": ("5000x3", 2.5e-3, 100, 1, 5, 16),
          "refits_3e-3": ("5000x3", 3e-3, 100, 1, 5, 16), "refine_0": ("5000x3", 2e-3, 100, 1, 0, 16), "refine_1": ("5000x3", 2e-3, 100, 1, 1, 16),
          "refine_16": ("5000x3", 2e-3, 100, 1, 16, 16), "general_K": ("300x8", THRESHOLD, 512, 1, 5, 2)}
TRACE_NAMES = tuple(n for n in LIMITS if n != "general_K")
# the traces the issue lists, per camera (accepted, changed, end) at 16 refits
LIMIT_TRACES = {"refits_1.2e-3": [(7, 7, "rejected"), (5, 5, "rejected"), (9, 9, "rejected")],
                "refits_2.5e-3": [(16, 4, "exhausted"), (3, 3, "rejected"), (16, 5, "exhausted")],
                "refits_3e-3": [(16, 2, "exhausted"), (1, 1, "rejected"), (2, 2, "rejected")],
                "refine_0": [(16, 0, "exhausted")] * 3,
                "refine_1": [(3, 3, "rejected"), (16, 6, "exhausted"), (3, 3, "rejected")],
                "refine_16": [(3, 3, "rejected")] * 3}
# Host-versus-host figure of a limit case (the rule of POSE_HOST_DIFF), measured by test_pose_ransac_cpu.py.  A trace case is ONE
# case, the same iteration cut at five places: its figure is the largest over the n_refit of LIMIT_REFIT_COUNTS with refits
# (REFIT_TRACE_DIFF's rule); without refits every trace case returns the same unrefitted best hypotheses: LIMIT_REFIT0_DIFF.
# ("refine_0" never moves a pose: its refits keep that figure.)
LIMIT_HOST_DIFF = {"refits_1.2e-3": 2.1e-10, "refits_2.5e-3": 1.5e-10, "refits_3e-3": 1.2e-10, "refine_0": 9.8e-15, "refine_1": 2.3e-10,
                   "refine_16": 8.8e-10, "general_K": 1.2e-9}
LIMIT_REFIT0_DIFF = 9.8e-15
# the smallest |d^2 / threshold^2 - 1| of a limit case over both routes and, for a trace case, over LIMIT_REFIT_COUNTS
LIMIT_MARGIN = {"refits_1.2e-3": 2.2e-5, "refits_2.5e-3": 1.1e-5, "refits_3e-3": 9.0e-6, "refine_0": 1.1e-5, "refine_1": 1.1e-5, "refine_16": 1.1e-5,
                "general_K": 1.0e-4}
Q_AXIS, K_SCALE = (0.2, -0.15, 0.1), 2.5  # "general_K": K' = 2.5 K Rod(Q_AXIS), a full matrix with K'[2][2] != 1
# "general_K" against "300x8" on the reference: max |t' - t| and max |R' - R Q| (K' R'^T = 2.5 K R^T: one camera matrix up to scale)
GENERAL_K_T_DIFF, GENERAL_K_R_DIFF = 5.3e-10, 9.7e-11


def general_K(K):
    return K_SCALE * (np.asarray(K) @ PR.rodrigues(np.array(Q_AXIS)))


@functools.lru_cache(maxsize=None)
def limit_case(name):
    """(X, pt_ptr, cam_idx, xy, K, threshold, n_hypotheses, seed, n_refine, n_refit) of a structural-limit case."""
    scene, thr, H, seed, n_refine, n_refit = LIMITS[name]
    X, pt_ptr, cam, xy, K = case(scene)[:5]
    if name == "general_K":
        K = general_K(K)
        K.setflags(write=False)
    return X, pt_ptr, cam, xy, K, thr, H, seed, n_refine, n_refit


@functools.lru_cache(maxsize=None)
def limit_reference(name, roots="roots", solver="chol", n_refit=None):
    X, pt_ptr, cam, xy, K, thr, H, seed, n_refine, r = limit_case(name)
    return PR.pose_robust(X, pt_ptr, cam, xy, K, thr, n_hyp=H, seed=seed, n_refine=n_refine, n_refit=r if n_refit is None else n_refit,
                          roots=roots, solver=solver)


def limit_margin(name, n_refit):
    """The parity margin of a limit case at ``n_refit``."""
    return MARGIN * (LIMIT_REFIT0_DIFF if n_refit == 0 and name in TRACE_NAMES else LIMIT_HOST_DIFF[name])


# "tiles_edges": the "edges" shape (257 / 256 / 255 observations: 2, 1 and 1 chunks) listed over and over at 65 536 hypotheses, so
# that the second tile starts at an entry whose chunk offset is not its list position
TILE_HYP = 65536
TILE_CAMERAS = (0, 1, 2) * 4
CHUNK, list_chunks, tile_sums = QC.CHUNK, QC.list_chunks, QC.tile_sums


# mvba_pose_refine at its limits: name -> n_steps of refine_case(); chol against lstsq (REFINE_HOST_DIFF's rule)
REFINE_STEP_COUNTS = (1, 2, 64)
REFINE_LIMIT_HOST_DIFF = {"steps_1": 5.7e-15, "steps_2": 8.9e-16, "steps_64": 2.9e-10, "general_K": 2.9e-10, "masks": 3.4e-11,
                          "masks_point_ok": 2.6e-11, "empty": 2.9e-10}
# ("statuses_a" / "statuses_b": exact data at the ground truth; neither route accepts a step, the figure is 0 and sets no margin)
MASK_STEPS = 10
POINT_DROP = 0.3
MASK_USABLE = {"masks": [1875, 1854, 1869], "masks_point_ok": [1414, 1411, 1411]}
STATUS_PIVOT_BOUND = 1e-14  # the failing relative pivots of "statuses_a" are below this or negative (the rule is 1e-12)
# measured on the reference: the failing pivot of the 40 collinear points (three collinear points: the factorisation meets a
# pivot that is not positive), and the smallest relative pivot of the camera with three observations (status 0)
STATUS_FAIL_PIVOT, STATUS_MIN_PIVOT = 1.6e-15, 1.2e-3


def _perturbed(sc, m):
    """Ground-truth poses perturbed as in refine_case()."""
    rng = np.random.default_rng(5)
    t0 = sc.t_gt + rng.normal(0.0, REFINE_PERTURBATION, sc.t_gt.shape)
    R0 = np.stack([PR.rodrigues(w) for w in rng.normal(0.0, REFINE_PERTURBATION, (m, 3))]) @ sc.R_gt
    return R0, t0


def chunk_pattern(n, seed=11):
    """(n,) bool over a camera's run: its 256-chunks cycle all / none / the last lane alone / a seeded half."""
    kind, lane = (np.arange(n) // CHUNK) % 4, np.arange(n) % CHUNK
    return (kind == 0) | ((kind == 2) & (lane == CHUNK - 1)) | ((kind == 3) & (np.random.default_rng(seed).random(n) < 0.5))


@functools.lru_cache(maxsize=None)
def refine_limit_case(name):
    """(X, pt_ptr, cam_idx, xy, K, R0, t0, point_ok, obs_ok, n_steps) of a pose_refine limit case:
    "steps_<n>": refine_case() at n_steps = n;  "general_K": refine_case() under K' = general_K(K), R0' = R0 Q;
    "masks": the clean "5000x3" list, obs_ok by chunk_pattern over each camera's run (20 chunks, the last of 136);
    "masks_point_ok": the same with a seeded 30 % of the points dropped by point_ok as well;
    "statuses_a" / "statuses_b": 80 points x 3 cameras without noise, the first 40 on one line, ground-truth poses; obs_ok
    leaves camera 0 everything, camera 1 the 40 collinear points / three points off the line, camera 2 three collinear / two points;
    "empty": refine_case() re-indexed into 11 cameras with 1, 4 and 10 unobserved (identity K and pose there)."""
    if name.startswith("steps_"):
        return refine_case() + (None, None, int(name[6:]))
    if name == "general_K":
        X, pt_ptr, cam, xy, K, R0, t0 = refine_case()
        return X, pt_ptr, cam, xy, general_K(K), R0 @ PR.rodrigues(np.array(Q_AXIS)), t0, None, None, REFINE_STEPS
    if name in ("masks", "masks_point_ok"):
        K, sc = true_K("5000x3")
        R0, t0 = _perturbed(sc, 3)
        pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
        ok = None if name == "masks" else np.random.default_rng(13).random(sc.n_points) >= POINT_DROP
        obs_ok = np.zeros(len(sc.cam_idx), bool)
        for k in range(3):  # a camera's run: its usable observations in ascending point order
            run = np.nonzero((sc.cam_idx == k) & (True if ok is None else ok[pt]))[0]
            obs_ok[run] = chunk_pattern(len(run), 11 + k)
        return sc.X_gt, sc.pt_ptr, sc.cam_idx, sc.xy, K, R0, t0, ok, obs_ok, MASK_STEPS
    if name in ("statuses_a", "statuses_b"):
        K, sc = true_K("coplanar")
        X = sc.X_gt.copy()
        X[:40] = sc.X_gt[0] + np.linspace(-1.0, 1.0, 40)[:, None] * np.array([0.3, 0.5, 0.2])
        pt = np.repeat(np.arange(80), np.diff(sc.pt_ptr))
        keep = {"statuses_a": (range(80), range(40), (3, 17, 31)), "statuses_b": (range(80), (40, 41, 42), (40, 41))}[name]
        obs_ok = np.zeros(len(pt), bool)
        for k in range(3):
            obs_ok |= (sc.cam_idx == k) & np.isin(pt, list(keep[k]))
        return X, sc.pt_ptr, sc.cam_idx, IC.exact_xy(sc, X), K, sc.R_gt, sc.t_gt, None, obs_ok, REFINE_STEPS
    if name == "empty":
        X, pt_ptr, cam, xy, m, kept = IC.empty_camera_case()
        _, _, _, _, K8, R8, t8 = refine_case()
        K, R0, t0 = np.tile(np.eye(3), (m, 1, 1)), np.tile(np.eye(3), (m, 1, 1)), np.zeros((m, 3))
        K[kept], R0[kept], t0[kept] = K8, R8, t8
        return X, pt_ptr, cam, xy, K, R0, t0, None, None, REFINE_STEPS
    raise KeyError(name)


REFINE_LIMIT_NAMES = ("steps_1", "steps_2", "steps_64", "general_K", "masks", "masks_point_ok", "statuses_a", "statuses_b", "empty")
STATUS_WANT = {"statuses_a": [0, 2, 2], "statuses_b": [0, 0, 1]}


@functools.lru_cache(maxsize=None)
def refine_limit_reference(name, solver="chol"):
    """(R, t, quality, n_usable, status, records) of the reference on a pose_refine limit case."""
    X, pt_ptr, cam, xy, K, R0, t0, ok, obs_ok, n_steps = refine_limit_case(name)
    out = PR.pose_refine(X, pt_ptr, cam, xy, K, R0, t0, point_ok=ok, obs_ok=obs_ok, n_steps=n_steps, solver=solver, trace=True)
    for a in out[:5]:
        a.setflags(write=False)
    return out
