"""Scenes shared by test_twoview_cpu.py and test_gpu_twoview.py, each built once, and the host-versus-host differences (eigh
of the moment matrix against the SVD of the stacked rows) that set the parity margins -- the rule of tests/_init_cases.py.
Test infrastructure only."""
import functools

import numpy as np

import _init_cases as IC
import _twoview_ref as T
from lib.synthetic import make_scene, project_obs

# Host-versus-host max-abs difference of F (|F| = 1) over the pairs of status 0, measured by test_twoview_cpu.py on the very
# scenes below.  A GPU parity assert gets MARGIN x its scene's figure; the Sampson RMS gets the same margin relative to its
# own size (|dq| <= margin x q).  "65x12" has pairs with exactly 8 shared points and lambda_1 / lambda_2 up to 0.04.
TWOVIEW_HOST_DIFF = {"300x8": 8.7e-14, "5000x3": 3.9e-15, "257x2": 2.1e-15, "65x12": 2.0e-11, "pixels": 9.2e-15,
                     "16641x3": 3.0e-15}
MARGIN = 100.0
# The noise-free 300 x 8 scene, pair (0, 1): the reference's F against the ground-truth essential matrix, its relative pose
# against the ground truth, and the host-versus-host difference of F there (all max abs, measured by test_twoview_cpu.py).
# The pose assert on the GPU gets MARGIN x the F figure x the factor by which the pose error exceeds the F error on the host.
POSE_F_HOST_DIFF, POSE_REF_F_ERR, POSE_REF_POSE_ERR = 5.6e-16, 1.8e-15, 1.0e-15


def pose_margin():
    return MARGIN * POSE_F_HOST_DIFF * max(1.0, POSE_REF_POSE_ERR / POSE_REF_F_ERR)


def all_pairs(m):
    return np.array([(k, l) for k in range(m) for l in range(k + 1, m)], np.int32)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "300x8":  # the issue's scene: 67 .. 90 shared points per pair
        return make_scene(300, 8, vis_p=0.5, project="numpy")
    if name == "5000x3":  # 20 chunks of 256 points per pair
        return make_scene(5000, 3, vis_p=1.0, project="numpy")
    if name == "257x2":  # the minimum camera count, more than one workgroup
        return make_scene(257, 2, vis_p=1.0, project="numpy")
    if name == "65x12":  # few shared points: 1 .. 11 per pair
        return make_scene(65, 12, vis_p=0.3, project="numpy")
    if name == "noise_free":
        return make_scene(300, 8, vis_p=0.5, noise=0.0, project="numpy")
    if name == "16641x3":  # dense; 66 chunks of 256 points, the last of one point: lanes 0 and 1 of the combine add two chunks each
        return make_scene(16641, 3, vis_p=1.0, project="numpy")
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """(pt_ptr, cam_idx, xy, n_images, pairs) of a parity shape; every pair k < l, and two reversed ones on 300x8."""
    if name == "pixels":  # f0 = 600, u = (320, 240): raw pixel observations
        sc, xy_px, _, _ = IC.pixel_scene()
        return sc.pt_ptr, sc.cam_idx, xy_px, 8, all_pairs(8)
    sc = scene(name)
    pairs = all_pairs(sc.n_images)
    if name == "300x8":
        pairs = np.concatenate([pairs, np.array([(5, 2), (7, 0)], np.int32)])
    if name == "16641x3":  # the six ordered pairs
        pairs = np.concatenate([pairs, pairs[:, ::-1]])
    return sc.pt_ptr, sc.cam_idx, sc.xy, sc.n_images, pairs


@functools.lru_cache(maxsize=None)
def reference(name, linear="eigh"):
    out = T.two_view(*case(name), linear=linear)
    for v in out:
        v.setflags(write=False)
    return out


TV_CHUNK, TV_PART_BYTES, TV_MAX_TILE = 256, 128 << 20, 65535  # csrc/mvba_twoview.h: points per chunk, bytes of partials per launch, gridDim.y


def pair_tile(n_points, n_pairs):
    """The number of pairs mvba_two_view takes per launch ("Partials")."""
    n_chunks = -(-n_points // TV_CHUNK)
    return max(1, min(n_pairs, TV_MAX_TILE, TV_PART_BYTES // (8 * 45 * n_chunks)))


def cycled(pairs, n):
    """The pair list repeated to length n."""
    return np.ascontiguousarray(np.resize(pairs, (n, 2)))


def no_shared_case():
    """The "300x8" list with a ninth camera that observes nothing: pair (0, 8) shares no point.  (pt_ptr, cam_idx, xy, 9)."""
    pt_ptr, cam, xy, _, _ = case("300x8")
    return pt_ptr, cam, xy, 9


def count_cases():
    """(pt_ptr, cam_idx, n_images, n_points) of the co-visibility shapes: sparse, degree above a wave's width, dense grid."""
    a, b = scene("300x8"), make_scene(65, 70, vis_p=1.0, project="numpy")
    return {"300x8": (a.pt_ptr, a.cam_idx, 8, 300), "65x70": (b.pt_ptr, b.cam_idx, 70, 65), "dense": (None, None, 5, 130)}


@functools.lru_cache(maxsize=None)
def degenerate_case(name):
    """(pt_ptr, cam_idx, xy, n_images, pair) of a noise-free pair whose moment matrix has a null space of dimension 3."""
    if name == "planar":  # every point in the plane z = 0
        sc = make_scene(80, 3, vis_p=1.0, noise=0.0, project="numpy")
        X = sc.X_gt.copy()
        X[:, 2] = 0.0
        return sc.pt_ptr, sc.cam_idx, IC.exact_xy(sc, X), 3, (0, 1)
    if name == "same_centre":  # cameras 2 and 3 at one centre, rotated against each other
        K, R, t, _, _, _, _, X = IC.status_case()
        pt, cam = np.repeat(np.arange(40), 4), np.tile(np.arange(4, dtype=np.int32), 40)
        xy = project_obs(X, K[:, 0, 0], K[:, :2, 2], t, R, 1.0, pt, cam)
        return np.arange(0, 164, 4, dtype=np.int64), cam, xy, 4, (2, 3)
    raise KeyError(name)


def true_essential(sc, k, l):
    """E with x_l^T E x_k = 0 for K = I cameras, |E| = 1, largest entry positive."""
    Rrel = sc.R_gt[l].T @ sc.R_gt[k]
    tau = sc.R_gt[l].T @ (sc.t_gt[k] - sc.t_gt[l])
    E = np.array([[0, -tau[2], tau[1]], [tau[2], 0, -tau[0]], [-tau[1], tau[0], 0]]) @ Rrel
    E = E / np.linalg.norm(E)
    return -E if E.flat[np.argmax(np.abs(E))] < 0 else E


def true_relative_pose(sc, k, l):
    """(R_l, t_l) with camera k at the origin with identity pose and |t_l| = 1."""
    b = sc.R_gt[k].T @ (sc.t_gt[l] - sc.t_gt[k])
    return sc.R_gt[k].T @ sc.R_gt[l], b / np.linalg.norm(b)


@functools.lru_cache(maxsize=None)
def short_camera_scene(which):
    """make_scene(300, 8, 0.5) with camera ``which`` cut down to 9 observations (fewer than min_points = 12)."""
    sc = scene("300x8")
    keep = np.ones(sc.n_obs, bool)
    keep[np.nonzero(sc.cam_idx == which)[0][9:]] = False
    pt = np.repeat(np.arange(300), np.diff(sc.pt_ptr))
    pt_ptr = np.concatenate([[0], np.cumsum(np.bincount(pt[keep], minlength=300))]).astype(np.int64)
    return pt_ptr, sc.cam_idx[keep], sc.xy[keep]
