"""Scenes shared by test_init_cpu.py and test_gpu_init.py, each built once: the parity shapes, the constructed status cases,
and the host-versus-host differences (eigh of the moment matrix against the SVD of the stacked rows) that set the parity
margins.  Test infrastructure only."""
import functools

import numpy as np

import _init_ref as ref
from lib.synthetic import make_scene, project_obs

# Host-versus-host differences of the LINEAR step, measured by test_init_cpu.py on the very scenes below (max abs; point
# coordinates of order 1, camera matrices with |P[2, :3]| = 1).  A GPU parity assert gets 100 x its scene's figure, for
# n_refine = 0 and 2 alike (a refined point is no better determined than the eigenvector it started from; after two steps
# the two host routes agree to 4e-16, which measures the convergence, not the arithmetic).
TRI_HOST_DIFF = {"300x8": 1.3e-14, "65x70": 1.6e-15, "257x2": 1.5e-14, "dense": 1.6e-15, "pixels": 1.2e-14, "300x683": 8.2e-15,
                 "300x1704": 1.2e-14}
RESECT_HOST_DIFF = {"300x8": 2.5e-14, "5000x3": 1.2e-14, "six": 1.2e-13, "dense": 2.4e-14, "900x300": 4.5e-13, "edges": 4.9e-14}
MARGIN = 100.0


@functools.lru_cache(maxsize=None)
def tri_scene(name):
    """(scene, xy for the call, pt_ptr / cam_idx or None) of a triangulation parity shape."""
    if name == "300x8":  # degrees 3 .. 8, a point count that is no multiple of 64 or 256
        return make_scene(300, 8, vis_p=0.5, project="numpy")
    if name == "65x70":  # degree above one wave's width
        return make_scene(65, 70, vis_p=1.0, project="numpy")
    if name == "257x2":  # the minimum degree, m = 2, more than one workgroup
        return make_scene(257, 2, vis_p=1.0, project="numpy")
    if name == "dense":  # the dense grid (pt_ptr = None)
        return make_scene(130, 5, vis_p=1.0, project="numpy")
    if name == "pixels":  # the 300 x 8 scene in pixel units: f0 = 600, f ~ 600, principal point (320, 240)
        return make_scene(300, 8, vis_p=0.5, project="numpy")
    # the LDS camera table (96 B per camera) above 64 KiB and at its cap; vis_p = 0.02 leaves the reference alone with status
    # 0 for 300 of 300 points in both (degrees 3 .. 23 and 18 .. 50)
    if name == "300x683":  # 65 568 B; 7 points observe camera 682, the row that crosses 64 KiB
        return make_scene(300, 683, vis_p=0.02, project="numpy")
    if name == "300x1704":  # 163 584 B, the cap; 3 points observe camera 1703, 6 camera 682, 6 camera 683
        return make_scene(300, 1704, vis_p=0.02, project="numpy")
    raise KeyError(name)


PIXEL_F0, PIXEL_U = 600.0, np.array([320.0, 240.0])


def pixel_scene(noise_free=False):
    """The 300 x 8 scene as a camera with f0 = 600 sees it: raw xy in pixels, and what BundleAdjuster takes for it --
    init_K = [[f,0,u],[0,f,v],[0,0,f0]] with f ~ 600, u = (320, 240).  (scene, xy_px, init_K, K_raw): K_raw is init_K with
    K[2, 2] = 1, the matrix that projects to the raw pixels.  noise_free: exact observations through the ground-truth cameras
    (K_gt scaled the same way) instead of the noisy ones through the perturbed cameras."""
    sc = make_scene(300, 8, vis_p=0.5, noise=0.0, project="numpy") if noise_free else tri_scene("pixels")
    Ku = sc.K_gt if noise_free else sc.init_K
    xy_px = PIXEL_F0 * (exact_xy(sc) if noise_free else sc.xy) + PIXEL_U
    K = np.zeros((8, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = PIXEL_F0 * Ku[:, 0, 0]
    K[:, :2, 2] = PIXEL_U
    K[:, 2, 2] = PIXEL_F0
    K_raw = K.copy()
    K_raw[:, 2, 2] = 1.0
    return sc, xy_px, K, K_raw


def tri_args(name):
    """(K, R, t, pt_ptr, cam_idx, xy) as the library takes them (the scene's perturbed initial cameras)."""
    sc = tri_scene(name)
    if name == "pixels":
        sc, xy_px, _, K_raw = pixel_scene()
        return K_raw, sc.init_R, sc.init_t, sc.pt_ptr, sc.cam_idx, xy_px
    if name == "dense":
        return sc.init_K, sc.init_R, sc.init_t, None, None, sc.xy.reshape(sc.n_points, sc.n_images, 2)
    return sc.init_K, sc.init_R, sc.init_t, sc.pt_ptr, sc.cam_idx, sc.xy


@functools.lru_cache(maxsize=None)
def tri_reference(name, n_refine, linear="eigh"):
    out = ref.triangulate(*tri_args(name), n_refine=n_refine, linear=linear)
    for v in out:
        v.setflags(write=False)
    return out


def exact_xy(sc, X=None):
    """Noise-free observations of a scene's list through its ground-truth cameras."""
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    return project_obs(sc.X_gt if X is None else X, sc.K_gt[:, 0, 0], sc.K_gt[:, :2, 2], sc.t_gt, sc.R_gt, 1.0, pt, sc.cam_idx)


@functools.lru_cache(maxsize=None)
def status_case():
    """40 points x 4 cameras, noise-free, cameras 2 and 3 at the same centre.  Point 3 is seen once (status 1), point 7 by
    cameras 2 and 3 only (no parallax: 2), point 11's two observations are those of a direction (at infinity: 3); every
    other point is seen by cameras 0, 1, 2.  Returns (K, R, t, pt_ptr, cam_idx, xy, expected status, X_gt)."""
    sc = make_scene(40, 4, vis_p=1.0, noise=0.0, project="numpy")
    K, R, t = sc.K_gt.copy(), sc.R_gt.copy(), sc.t_gt.copy()
    c, s = np.cos(0.3), np.sin(0.3)
    t[3] = t[2]
    R[3] = R[2] @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    cams = {a: [0, 1, 2] for a in range(40)}
    cams[3], cams[7], cams[11] = [0], [2, 3], [0, 1]
    pt = np.concatenate([np.full(len(cams[a]), a) for a in range(40)])
    cam = np.concatenate([cams[a] for a in range(40)]).astype(np.int32)
    xy = project_obs(sc.X_gt, K[:, 0, 0], K[:, :2, 2], t, R, 1.0, pt, cam)
    d = np.array([0.2, -0.1, -1.0])  # a direction in front of cameras 0 and 1 (they look at the origin from x > 0 ... any non-zero depth does)
    sel = pt == 11
    p = np.einsum("oij,j->oi", K[cam[sel]] @ np.transpose(R[cam[sel]], (0, 2, 1)), d)
    xy[sel] = p[:, :2] / p[:, 2:3]
    pt_ptr = np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=40))]).astype(np.int64)
    expect = np.zeros(40, np.int32)
    expect[3], expect[7], expect[11] = 1, 2, 3
    return K, R, t, pt_ptr, cam, xy, expect, sc.X_gt


@functools.lru_cache(maxsize=None)
def resect_case(name):
    """(X, pt_ptr, cam_idx, xy, n_images, expected status) of a resection parity shape."""
    if name == "300x8":
        sc = tri_scene("300x8")
        return sc.X_gt, sc.pt_ptr, sc.cam_idx, sc.xy, 8, np.zeros(8, np.int32)
    if name == "5000x3":  # 5000 observations per camera: 20 chunks of 256
        sc = make_scene(5000, 3, vis_p=1.0, project="numpy")
        return sc.X_gt, sc.pt_ptr, sc.cam_idx, sc.xy, 3, np.zeros(3, np.int32)
    if name == "six":  # camera 1 keeps exactly 6 observations (status 0), camera 2 keeps 5 (status 1); noise-free
        sc = make_scene(60, 4, vis_p=1.0, noise=0.0, project="numpy")
        pt = np.repeat(np.arange(60), 4)
        keep = ~(((sc.cam_idx == 1) & (pt >= 6)) | ((sc.cam_idx == 2) & (pt >= 5)))
        pt_ptr = np.concatenate([[0], np.cumsum(np.bincount(pt[keep], minlength=60))]).astype(np.int64)
        return sc.X_gt, pt_ptr, sc.cam_idx[keep], sc.xy[keep], 4, np.array([0, 0, 1, 0], np.int32)
    if name == "dense":  # the dense grid (pt_ptr = None from Python): 130 x 5, every camera sees every point
        sc = tri_scene("dense")
        return sc.X_gt, sc.pt_ptr, sc.cam_idx, sc.xy, 5, np.zeros(5, np.int32)
    if name == "coplanar":  # every point in the plane z = 0: the DLT has a four-dimensional null space (status 2)
        sc = make_scene(80, 3, vis_p=1.0, noise=0.0, project="numpy")
        X = sc.X_gt.copy()
        X[:, 2] = 0.0
        return X, sc.pt_ptr, sc.cam_idx, exact_xy(sc, X), 3, np.full(3, 2, np.int32)
    if name == "900x300":  # more than 256 cameras (k_resect_norm beyond one workgroup), 38 .. 76 observations each: none below 6
        sc = make_scene(900, 300, vis_p=0.06, project="numpy")
        return sc.X_gt, sc.pt_ptr, sc.cam_idx, sc.xy, 300, np.where(np.bincount(sc.cam_idx, minlength=300) < 6, 1, 0).astype(np.int32)
    if name == "edges":  # 257 observations for camera 0 (a chunk of one after a full one), 256 for camera 1 (a full chunk), 255 for camera 2
        sc = make_scene(257, 3, vis_p=1.0, project="numpy")
        pt = np.repeat(np.arange(257), 3)
        keep = ~(((sc.cam_idx == 1) & (pt >= 256)) | ((sc.cam_idx == 2) & (pt >= 255)))
        pt_ptr = np.concatenate([[0], np.cumsum(np.bincount(pt[keep], minlength=257))]).astype(np.int64)
        return sc.X_gt, pt_ptr, sc.cam_idx[keep], sc.xy[keep], 3, np.zeros(3, np.int32)
    raise KeyError(name)


GRID_CAP = 2048 * 256  # the grid of k_triangulate and k_covisibility: at most 2048 workgroups of 256 threads, then grid-stride


@functools.lru_cache(maxsize=None)
def tiled_scene():
    """The "300x8" list repeated along the point axis until it passes GRID_CAP by a few whole tiles (1754 tiles, 526 200
    points): (reps, pt_ptr, cam_idx, xy).  The cameras stay those of tri_args("300x8")."""
    sc = tri_scene("300x8")
    reps = GRID_CAP // sc.n_points + 7
    deg = np.tile(np.diff(sc.pt_ptr), reps)
    pt_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    out = reps, pt_ptr, np.tile(sc.cam_idx, reps), np.tile(sc.xy, (reps, 1))
    for v in out[1:]:
        v.setflags(write=False)
    return out


EMPTY_CAMERAS = (1, 4, 10)


def empty_camera_case():
    """The "300x8" list re-indexed into m = 11 with cameras 1, 4 and 10 unobserved: (X, pt_ptr, cam_idx, xy, 11, kept) with
    kept[j] the new index of the old camera j."""
    X, pt_ptr, cam, xy, _, _ = resect_case("300x8")
    kept = np.array([k for k in range(11) if k not in EMPTY_CAMERAS], np.int32)
    return X, pt_ptr, kept[cam], xy, 11, kept


COINCIDENT_CAMERA = 3
# the image point a camera's observations are collapsed onto: sums of the first are exact in binary floating point (the
# centroid is the point itself, the spread exactly 0, the Hartley scale infinite, inf x 0 = NaN in the second pass); the
# second is not representable, so the centroid may miss it by one ulp (a finite scale of the order 1e17 and identical
# normalised points: a null space of dimension 4 for the DLT, 6 for the epipolar rows)
COINCIDENT_POINTS = {"exact": (0.25, -0.5), "inexact": (0.1, 0.3)}


def coincident_xy(kind):
    """The xy of "300x8" with every observation of COINCIDENT_CAMERA at one image point."""
    sc = tri_scene("300x8")
    xy = sc.xy.copy()
    xy[sc.cam_idx == COINCIDENT_CAMERA] = COINCIDENT_POINTS[kind]
    return xy


def duplicate_observation_case():
    """status_case() with point 5 observed by camera 2 twice, the same image point both times (no parallax: status 2); the
    run [2, 2] does not ascend, which the stateless call does not ask for.  (K, R, t, pt_ptr, cam_idx, xy, expected)."""
    K, R, t, pt_ptr, cam, xy, expect, _ = status_case()
    keep = np.ones(len(cam), bool)
    keep[pt_ptr[5]] = False  # drop camera 0; then camera 1 becomes the copy of camera 2
    cam, xy = cam.copy(), xy.copy()
    cam[pt_ptr[5] + 1], xy[pt_ptr[5] + 1] = 2, xy[pt_ptr[5] + 2]
    deg = np.diff(pt_ptr)
    deg[5] = 2
    expect = expect.copy()
    expect[5] = 2
    return K, R, t, np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), cam[keep], xy[keep], expect


@functools.lru_cache(maxsize=None)
def resect_reference(name, linear="eigh"):
    X, pt_ptr, cam_idx, xy, m, _ = resect_case(name)
    out = ref.resect(X, pt_ptr, cam_idx, xy, m, linear=linear)
    for v in out:
        v.setflags(write=False)
    return out
