"""Scenes shared by test_ransac_cpu.py and test_gpu_ransac.py, each built once, with the contamination every robust test uses,
and the host-versus-host differences (eigh of the moment matrices against the SVD of the stacked rows) that set the parity
margins -- the rule of tests/_twoview_cases.py.  Test infrastructure only."""
import functools

import numpy as np

import _init_cases as IC
import _ransac_ref as RR
import _twoview_cases as C
import _twoview_ref as T
from lib.synthetic import make_scene

MARGIN = C.MARGIN
THRESHOLD = 0.01  # the median Sampson distance of clean points on these scenes is 6 - 7e-4
# Host-versus-host max-abs difference of the final F (|F| = 1) over the pairs of status 0, measured by test_ransac_cpu.py on
# the very cases below.  A GPU parity assert gets MARGIN x its case's figure; the Sampson RMS the same margin relative to
# its own size.
RANSAC_HOST_DIFF = {"300x8": 8.7e-14, "2000x3": 1.3e-14, "257x2": 7.8e-16, "dense130x3": 3.8e-15, "pixels": 9.2e-15,
                    # the structural limits (LIMITS below)
                    "scan257": 2.4e-15, "refits_1.5e-3": 4.0e-15, "refits_3e-3": 4.7e-15, "mixed": 5.1e-15, "mixed65": 3.6e-12,
                    "partly_degenerate": 6.1e-15}
# relative_pose on the contaminated 300x8 pair (0, 1): host-versus-host difference of the robust pose, the error of the
# UNcontaminated plain pose against the ground truth, and the errors of the robust and of the plain pose on the contaminated
# pair against the ground truth (all max abs over R_1 and t_1, measured by test_ransac_cpu.py)
POSE_HOST_DIFF, POSE_CLEAN_ERR, POSE_ROBUST_ERR, POSE_PLAIN_ERR = 2.3e-15, 6.6e-3, 8.2e-3, 1.7
POSE_FACTOR = 10.0  # the robust pose is within this factor of the uncontaminated pair's error
BOOT_FRACTION = 0.25  # of camera 1's observations replaced in the bootstrap case
BOOT_HOST_DIFF = 9.0e-13  # host-versus-host difference of the robust bootstrap's poses and points (max abs)


def contaminate(pt_ptr, cam_idx, xy, k, l, frac, seed=7):
    """(xy', bad): the pair's shared list with the image-l observation of each ``bad`` point replaced by a uniform position
    inside the bounds of all xy.  ``bad`` (n,) is over the shared points in ascending order."""
    xy = np.array(xy, np.float64).reshape(-1, 2)
    n = len(pt_ptr) - 1
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    ids = T.shared(pt_ptr, cam_idx, xy, k, l)[0]
    ol = np.full(n, -1)
    ol[pt[cam_idx == l]] = np.nonzero(cam_idx == l)[0]
    rng = np.random.default_rng(seed)
    bad = rng.random(len(ids)) < frac
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    xy[ol[ids[bad]]] = lo + rng.random((int(bad.sum()), 2)) * (hi - lo)
    return xy, bad


# name: (frac of pair (0, 1) replaced in image 1, n_hypotheses, seed)
PARITY = {"300x8": (0.3, 512, 1), "2000x3": (0.4, 100, 1), "257x2": (0.3, 1, 1), "dense130x3": (0.3, 64, 1), "pixels": (0.3, 512, 1)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses, seed, bad) of a parity case.  Pair (0, 1) is
    contaminated in image 1 (so every pair with camera 1 carries some of it); ``bad`` is over its shared list."""
    frac, H, seed = PARITY[name]
    thr = THRESHOLD
    if name == "pixels":  # f0 = 600: raw pixel observations, the threshold in pixels
        pt_ptr, cam, xy, m, pairs = C.case("pixels")
        thr = THRESHOLD * IC.PIXEL_F0
    elif name == "300x8":  # one chunk per pair; the compaction skips points (67 .. 90 of 300 are shared)
        pt_ptr, cam, xy, m, pairs = C.case("300x8")
    else:
        n, m = {"2000x3": (2000, 3), "257x2": (257, 2), "dense130x3": (130, 3)}[name]
        sc = make_scene(n, m, vis_p=1.0, project="numpy")
        pt_ptr, cam, xy, pairs = sc.pt_ptr, sc.cam_idx, sc.xy, C.all_pairs(m)
    xy, bad = contaminate(pt_ptr, cam, xy, 0, 1, frac)
    if name == "dense130x3":  # the dense grid: pt_ptr = None, xy (N, m, 2)
        pt_ptr, cam, xy = None, None, xy.reshape(130, 3, 2)
    for a in (xy, bad):
        a.setflags(write=False)
    return pt_ptr, cam, xy, m, pairs, thr, H, seed, bad


@functools.lru_cache(maxsize=None)
def reference(name, linear="eigh", n_refit=2):
    pt_ptr, cam, xy, m, pairs, thr, H, seed, _ = case(name)
    return RR.two_view_robust(pt_ptr, cam, xy, m, pairs, thr, H, seed, n_refit, linear)


@functools.lru_cache(maxsize=None)
def status_cases():
    """name: (pt_ptr, cam_idx, xy, n_images, pairs, expected status) of the status branches (n_hypotheses 16, seed 1).
    "all_replaced" has status 0, not 4: a minimal sample fits its own 8 points exactly, so a hypothesis that is not degenerate
    counts at least 8 at any threshold above rounding, and status 4 cannot be reached from data (test_ransac_cpu.py asserts
    this on every count table); what the case shows instead is a best count far below half of the shared points."""
    pt_ptr, cam, xy, m, pairs = C.case("65x12")
    ns = C.reference("65x12")[2]
    out = {"eight": (pt_ptr, cam, xy, m, pairs[ns == 8][:1], 0),  # every hypothesis draws the same 8 points
           "seven": (pt_ptr, cam, xy, m, pairs[ns == 7][:1], 1)}
    pt_ptr, cam, xy, m, pair = C.degenerate_case("planar")
    out["planar"] = (pt_ptr, cam, xy, m, np.array([pair], np.int32), 2)
    pt_ptr, cam, xy, m, pairs = C.case("300x8")
    out["all_replaced"] = (pt_ptr, cam, contaminate(pt_ptr, cam, xy, 0, 1, 2.0)[0], m, pairs[:1], 0)
    return out


# The structural limits ("Structural limits"): name: (n_hypotheses, seed, threshold, n_refit)
LIMITS = {"scan257": (64, 1, THRESHOLD, 16), "refits_1.5e-3": (100, 1, 1.5e-3, 16), "refits_3e-3": (100, 1, 3e-3, 16),
          "mixed": (64, 1, THRESHOLD, 2), "mixed65": (64, 1, THRESHOLD, 2), "partly_degenerate": (64, 1, THRESHOLD, 2)}
SCAN_POINTS = 65_700  # 257 chunks of 256 points: k_ransac_scan gives a thread two chunks, thread 128 one, threads 129 .. 255 none
MAX_HYP = 65536  # csrc/mvba_ransac_host.h: RS_MAX_HYP
REFIT_COUNTS = (0, 1, 2, 3, 16)  # the n_refit at which the "refits" cases run on the device


def scan_keep():
    """(SCAN_POINTS,) bool: the points camera 1 of "scan257" keeps.  The 256-point chunks cycle through all kept, none kept,
    the point at lane 255 alone, and a seeded random half (the last chunk, 164 points, is of the first kind)."""
    kind = (np.arange(SCAN_POINTS) // 256) % 4
    lane = np.arange(SCAN_POINTS) % 256
    half = np.random.default_rng(11).random(SCAN_POINTS) < 0.5
    return (kind == 0) | ((kind == 2) & (lane == 255)) | ((kind == 3) & half)


def chunk_counts(pt_ptr, cam, xy, k, l):
    """The number of shared points of pair (k, l) in each chunk of 256 points (cnt[] of k_ransac_count)."""
    n = len(pt_ptr) - 1
    ids = T.shared(pt_ptr, cam, np.asarray(xy).reshape(-1, 2), k, l)[0]
    return np.bincount(ids // 256, minlength=-(-n // 256))


@functools.lru_cache(maxsize=None)
def limit_case(name):
    """(pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses, seed, n_refit) of a structural-limit case."""
    H, seed, thr, n_refit = LIMITS[name]
    if name == "scan257":
        sc = make_scene(SCAN_POINTS, 3, vis_p=1.0, project="numpy")
        keep = np.ones((SCAN_POINTS, 3), bool)
        keep[:, 1] = scan_keep()
        keep = keep.reshape(-1)
        pt_ptr = np.concatenate([[0], np.cumsum(keep.reshape(-1, 3).sum(axis=1))]).astype(np.int64)
        cam, xy, m = sc.cam_idx[keep], sc.xy.reshape(-1, 2)[keep], 3
        pairs = np.array([(0, 1), (1, 2), (2, 1)], np.int32)  # ((0, 2) has a distance within 1e-7 of the threshold: left out)
        xy = contaminate(pt_ptr, cam, xy, 0, 1, 0.3)[0]
    elif name.startswith("refits"):  # the "2000x3" parity case at 16 refits and tighter thresholds: the inlier set moves
        pt_ptr, cam, xy, m, pairs = case("2000x3")[:5]
    elif name == "mixed":  # "300x8" plus an unobserved ninth camera, camera 3 collapsed onto one image point, pair (0, 1) contaminated
        pt_ptr, cam, _, m = C.no_shared_case()
        xy = contaminate(pt_ptr, cam, IC.coincident_xy("exact"), 0, 1, 0.3)[0]
        c = IC.COINCIDENT_CAMERA
        pairs = np.array([(0, 1), (0, 8), (c, 0), (5, 2), (8, 4), (1, c), (1, 2), (8, c), (c, 8), (6, 7), (c, 5), (4, 6), (7, 8), (2, 0)], np.int32)
    elif name == "mixed65":  # 1 .. 11 shared points per pair: status 1 WITH shared points next to status 0
        pt_ptr, cam, xy, m, all_ = C.case("65x12")
        ns = C.reference("65x12")[2]
        few, enough = all_[(ns >= 1) & (ns <= 7)], all_[ns >= 8]
        pairs = np.empty((2 * len(enough), 2), np.int32)
        pairs[0::2], pairs[1::2] = enough, few[np.linspace(0, len(few) - 1, len(enough)).astype(int)]
        pairs[3] = pairs[3, ::-1]
    elif name == "partly_degenerate":  # "300x8" pair (0, 2): 30 % of the shared points are copies of the first, in both images
        pt_ptr, cam, xy, m, _ = C.case("300x8")
        xy = np.array(xy, np.float64).reshape(-1, 2)
        ids = T.shared(pt_ptr, cam, xy, 0, 2)[0]
        dup = ids[np.random.default_rng(5).random(len(ids)) < 0.3]
        pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
        for c in (0, 2):
            obs = np.full(len(pt_ptr) - 1, -1)
            obs[pt[cam == c]] = np.nonzero(cam == c)[0]
            xy[obs[dup]] = xy[obs[ids[0]]]
        pairs = np.array([(0, 2)], np.int32)
    else:
        raise KeyError(name)
    xy = np.array(xy, np.float64)
    xy.setflags(write=False)
    return pt_ptr, cam, xy, m, pairs, thr, H, seed, n_refit


@functools.lru_cache(maxsize=None)
def limit_reference(name, linear="eigh", n_refit=None):
    pt_ptr, cam, xy, m, pairs, thr, H, seed, r = limit_case(name)
    return RR.two_view_robust(pt_ptr, cam, xy, m, pairs, thr, H, seed, r if n_refit is None else n_refit, linear)


def max_hyp_sample():
    """The h whose counts the n_hypotheses = MAX_HYP test compares with the reference: every 97th and the last 64."""
    return np.union1d(np.arange(0, MAX_HYP, 97), np.arange(MAX_HYP - 64, MAX_HYP))


@functools.lru_cache(maxsize=None)
def max_hyp_reference(linear="eigh"):
    """(h, counts, margin, pivot) of "300x8" pair (0, 1) at the h of max_hyp_sample()."""
    pt_ptr, cam, xy, m, pairs, thr, _, seed, _ = case("300x8")
    _, xk, xl = T.shared(pt_ptr, cam, np.asarray(xy).reshape(-1, 2), 0, 1)
    hs = max_hyp_sample()
    return (hs,) + RR.hypothesis_counts(xk, xl, 0, 1, thr, seed, hs, linear)


def end_refit(ref, n_refit):
    """The refit at which each pair of status 0 left the loop: the index of the rejected or failed one, or n_refit."""
    return np.where(ref["end"] == "exhausted", n_refit, ref["n_accepted"])


RS_POINT_BYTES, RS_HYP_BYTES = 48, 160  # csrc/mvba_ransac.h: device bytes per pair and point, per pair and hypothesis


def pair_tile(n_points, n_pairs, n_hyp):
    """The number of pairs mvba_two_view_robust takes per tile ("Tiles")."""
    return max(1, min(n_pairs, C.TV_MAX_TILE, C.TV_PART_BYTES // (RS_POINT_BYTES * n_points + RS_HYP_BYTES * n_hyp)))


@functools.lru_cache(maxsize=None)
def pose_case():
    """The contaminated 300x8 pair (0, 1), frac 0.3: (scene, xy', bad)."""
    sc = C.scene("300x8")
    xy, bad = contaminate(sc.pt_ptr, sc.cam_idx, sc.xy, 0, 1, 0.3)
    xy.setflags(write=False)
    return sc, xy, bad


def pose_error(sc, R, t, k=0, l=1):
    Rg, tg = C.true_relative_pose(sc, k, l)
    return max(np.abs(R[1] - Rg).max(), np.abs(t[1] - tg).max())


@functools.lru_cache(maxsize=None)
def reference_pose(linear="eigh"):
    sc, xy, _ = pose_case()
    return RR.relative_pose(sc.pt_ptr, sc.cam_idx, xy, sc.K_gt, (0, 1), THRESHOLD, 512, 1, linear=linear)


@functools.lru_cache(maxsize=None)
def bootstrap_case(frac=BOOT_FRACTION):
    """300x8 with ``frac`` of camera 1's observations replaced by uniform positions: (scene, xy', replaced (n_obs,) bool)."""
    sc = C.scene("300x8")
    xy = np.array(sc.xy, np.float64).reshape(-1, 2)
    obs = np.nonzero(sc.cam_idx == 1)[0]
    rng = np.random.default_rng(7)
    hit = obs[rng.random(len(obs)) < frac]
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    xy[hit] = lo + rng.random((len(hit), 2)) * (hi - lo)
    replaced = np.zeros(len(xy), bool)
    replaced[hit] = True
    xy.setflags(write=False)
    return sc, xy, replaced


@functools.lru_cache(maxsize=None)
def reference_bootstrap(frac=BOOT_FRACTION, linear="eigh"):
    from lib.initialization import engine_intrinsics

    sc, xy, _ = bootstrap_case(frac)
    return RR.bootstrap(sc.pt_ptr, sc.cam_idx, xy, engine_intrinsics(sc.init_K), THRESHOLD, 512, 1, linear=linear, start_pair=(0, 1), max_rms=0.01)
