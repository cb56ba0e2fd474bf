"""Scenes shared by test_resect_ransac_cpu.py and test_gpu_resect_ransac.py, each built once, with the contamination every test
of the robust resection uses, and the host-versus-host differences (eigh of the moment matrices against the SVD of the stacked
rows) that set the parity margins -- the rule of tests/_init_cases.py.  Test infrastructure only."""
import functools

import numpy as np

import _init_cases as IC
import _resect_ransac_ref as QR
import _twoview_ref as T

MARGIN = IC.MARGIN
THRESHOLD = 0.01  # ten times the noise of the scenes
# Host-versus-host max-abs difference of the final P (|P[2, :3]| = 1) over the cameras of status 0, measured by
# test_resect_ransac_cpu.py on the very cases below.  A GPU parity assert gets MARGIN x its case's figure; the RMS residual and
# the eigenvalue ratio get the same margin, absolutely (test_gpu_resect_ransac.py's docstring says why the RMS is not relative).
RESECT_RANSAC_HOST_DIFF = {"300x8": 5.6e-14, "5000x3": 3.2e-14, "edges_h1": 3.2e-13, "edges_h65": 2.7e-14, "dense": 5.4e-14, "pixels": 1.2e-11,
                           "900x300": 3.7e-12,
                           # n_refit = 0: the best MINIMAL-sample matrix (a 6-point DLT is far worse conditioned than the full fit)
                           "300x8_refit0": 8.0e-13,
                           # the status shapes (STATUS_NAMES below)
                           "six": 1.2e-13, "empty": 5.6e-14, "point_ok": 7.3e-14, "nan_X": 7.3e-14, "all_replaced": 5.6e-14}
# the same for the refit trace (refit_reference below), by n_refit
REFIT_HOST_DIFF = {0: 1.2e-11, 1: 1.7e-13, 2: 9.5e-14, 16: 1.7e-14}
# bootstrap with resect_threshold on the contaminated tracks of bootstrap_case(): host-versus-host difference of poses and
# points (max abs), the pose error of the UNcontaminated plain bootstrap against the ground truth, and that of the robust
# bootstrap on the contaminated tracks (max abs over R and t of the registered cameras, in the output frame; measured by
# test_resect_ransac_cpu.py)
BOOT_HOST_DIFF, BOOT_CLEAN_ERR, BOOT_ROBUST_ERR = 2.0e-12, 2.8e-2, 3.1e-2
# the robust bootstrap's poses are within this factor of the uncontaminated bootstrap's error: it resects from about 70 % of the
# observations the clean run has (1 / sqrt(0.7) = 1.2) and keeps 251 of 300 points
BOOT_FACTOR = 2.0
BOOT_FRACTION = 0.2  # of the observations of cameras 2 .. 7 replaced in the bootstrap case


def contaminate(cam_idx, xy, frac, seed=7, cameras=None):
    """(xy', replaced (n_obs,) bool): a seeded fraction ``frac`` of each camera's observations (of ``cameras``; default all)
    replaced by uniform positions inside the bounds of all xy."""
    xy = np.array(xy, np.float64).reshape(-1, 2)
    rng = np.random.default_rng(seed)
    hit = rng.random(len(xy)) < frac
    if cameras is not None:
        hit &= np.isin(cam_idx, cameras)
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    xy[hit] = lo + rng.random((int(hit.sum()), 2)) * (hi - lo)
    return xy, hit


# name: (resection shape of _init_cases.resect_case, fraction replaced, n_hypotheses, seed)
PARITY = {"300x8": ("300x8", 0.3, 512, 1), "5000x3": ("5000x3", 0.4, 100, 1), "edges_h1": ("edges", 0.3, 1, 1),
          "edges_h65": ("edges", 0.3, 65, 1), "dense": ("dense", 0.3, 64, 1), "pixels": ("300x8", 0.3, 512, 1), "900x300": ("900x300", 0.3, 64, 1)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, pt_ptr, cam_idx, xy, n_images, threshold, n_hypotheses, seed, f0, replaced) of a parity case."""
    shape, frac, H, seed = PARITY[name]
    X, pt_ptr, cam, xy, m, _ = IC.resect_case(shape)
    thr, f0 = THRESHOLD, 1.0
    if name == "pixels":  # f0 = 600: raw pixel observations, the threshold in pixels
        xy, thr, f0 = IC.pixel_scene()[1], THRESHOLD * IC.PIXEL_F0, IC.PIXEL_F0
    xy, hit = contaminate(cam, xy, frac)
    if name == "dense":  # the dense grid: pt_ptr = None, xy (N, m, 2)
        pt_ptr, cam, xy = None, None, xy.reshape(len(X), m, 2)
    for a in (xy, hit):
        a.setflags(write=False)
    return X, pt_ptr, cam, xy, m, thr, H, seed, f0, hit


@functools.lru_cache(maxsize=None)
def reference(name, linear="eigh", n_refit=2):
    X, pt_ptr, cam, xy, m, thr, H, seed, _, _ = case(name)
    return QR.resect_robust(X, pt_ptr, cam, xy, m, thr, n_hyp=H, seed=seed, n_refit=n_refit, linear=linear)


STATUS_HYP, STATUS_SEED = 16, 1
ALL_REPLACED_CAMERA = 3


@functools.lru_cache(maxsize=None)
def status_case(name):
    """(X, pt_ptr, cam_idx, xy, n_images, point_ok or None, expected status) of a status shape (n_hypotheses 16, seed 1)."""
    if name == "six":  # camera 1: exactly 6 usable observations, every hypothesis is the same set; camera 2: 5
        X, pt_ptr, cam, xy, m, want = IC.resect_case("six")
        return X, pt_ptr, cam, xy, m, None, want
    if name == "coplanar":  # every minimal sample lies in a plane
        X, pt_ptr, cam, xy, m, want = IC.resect_case("coplanar")
        return X, pt_ptr, cam, xy, m, None, want
    if name == "empty":  # cameras 1, 4 and 10 unobserved among observed ones
        X, pt_ptr, cam, xy, m, _ = IC.empty_camera_case()
        want = np.zeros(m, np.int32)
        want[list(IC.EMPTY_CAMERAS)] = 1
        return X, pt_ptr, cam, contaminate(cam, xy, 0.3)[0], m, None, want
    X, pt_ptr, cam, xy, m, _ = IC.resect_case("300x8")
    if name in ("point_ok", "nan_X"):  # a seeded 70 % of the points usable: by the mask, or by NaN in X
        ok = np.random.default_rng(3).random(len(X)) < 0.7
        xy = contaminate(cam, xy, 0.3)[0]
        if name == "point_ok":
            return X, pt_ptr, cam, xy, m, ok, np.zeros(m, np.int32)
        return np.where(ok[:, None], X, np.nan), pt_ptr, cam, xy, m, None, np.zeros(m, np.int32)
    if name == "all_replaced":  # every observation of camera 3 replaced, 30 % of the others'
        xy = contaminate(cam, xy, 0.3)[0]
        xy = contaminate(cam, xy, 2.0, seed=9, cameras=[ALL_REPLACED_CAMERA])[0]
        return X, pt_ptr, cam, xy, m, None, None  # (camera 3: whatever the reference says)
    raise KeyError(name)


STATUS_NAMES = ("six", "coplanar", "empty", "point_ok", "nan_X", "all_replaced")


@functools.lru_cache(maxsize=None)
def status_reference(name, linear="eigh"):
    X, pt_ptr, cam, xy, m, ok, _ = status_case(name)
    return QR.resect_robust(X, pt_ptr, cam, xy, m, THRESHOLD, point_ok=ok, n_hyp=STATUS_HYP, seed=STATUS_SEED, n_refit=2, linear=linear)


# the refit trace: "5000x3" at a threshold of twice the noise, where the inlier set moves from refit to refit
REFIT_THRESHOLD, REFIT_COUNTS = 2e-3, (0, 1, 2, 16)


@functools.lru_cache(maxsize=None)
def refit_reference(n_refit, linear="eigh"):
    X, pt_ptr, cam, xy, m, _, H, seed, _, _ = case("5000x3")
    return QR.resect_robust(X, pt_ptr, cam, xy, m, REFIT_THRESHOLD, n_hyp=H, seed=seed, n_refit=n_refit, linear=linear)


MAX_HYP = 65536  # csrc/mvba_ransac_host.h: RS_MAX_HYP
MAX_HYP_CAMERA = 0


def max_hyp_sample():
    """The h whose counts the n_hypotheses = MAX_HYP test compares with the reference: every 97th and the last 64."""
    return np.union1d(np.arange(0, MAX_HYP, 97), np.arange(MAX_HYP - 64, MAX_HYP))


@functools.lru_cache(maxsize=None)
def max_hyp_reference(linear="eigh"):
    """(h, counts, margin, pivot) of camera MAX_HYP_CAMERA of "300x8" at the h of max_hyp_sample()."""
    X, pt_ptr, cam, xy, m, thr, _, seed, _, _ = case("300x8")
    pt = np.repeat(np.arange(len(X)), np.diff(pt_ptr))
    obs = np.nonzero(cam == MAX_HYP_CAMERA)[0]
    hs = max_hyp_sample()
    return (hs,) + QR.hypothesis_counts(X[pt[obs]], np.asarray(xy)[obs], MAX_HYP_CAMERA, thr, seed, hs, linear)


TV_PART_BYTES, RR_HYP_BYTES, MAX_TILE = 128 << 20, 100, 65535  # csrc/mvba_twoview.h, csrc/mvba_resect_ransac.h


def camera_tile(n_cameras, n_hyp):
    """The number of cameras mvba_resect_robust takes per tile ("Tiles"): a restatement of the formula in Python.
    The library does not report its tile size, and results do not depend on it, so this says which calls MUST split if the C
    code follows the formula; it cannot show that the C code does."""
    return max(1, min(n_cameras, MAX_TILE, TV_PART_BYTES // (RR_HYP_BYTES * n_hyp)))


# "tiles_edges" (DESIGN.md 18): the "edges" shape (257 / 256 / 255 observations: 2, 1 and 1 chunks) listed 7 times at 65 536
# hypotheses -- 21 entries for a tile of 20, and the second tile starts at an entry whose chunk offset (27) is not its list
# position (20).  The device test is tests/test_gpu_pose_limits.py::test_two_tiles_of_the_dlt.
TILE_HYP = 65536
TILE_CAMERAS = (0, 1, 2) * 7
CHUNK = 256  # csrc/mvba_start.h: START_CHUNK


def list_chunks(cameras, n_usable):
    """lc_ch (len(cameras) + 1,) of CamChunks::build: the first chunk of each listed entry; n_usable is per camera of the scene."""
    return np.concatenate([[0], np.cumsum([-(-int(n_usable[k]) // CHUNK) for k in cameras])])


def tile_sums(cameras, n_usable, masks, tile, offset="chunk"):
    """n_inliers per list entry as the tile loop gets them: k_resect_mask writes a (count) partial per chunk of the tile into ONE
    buffer that the call keeps, from the tile's offset on, and k_resect_combine adds the entry's chunks lc_ch[c] .. lc_ch[c + 1]
    of that buffer.  ``masks[k]`` is camera k's final mask; ``offset`` = "chunk" is the code as written (the tile's chunks start
    at lc_ch[c0]), "camera" the deliberately wrong one (at c0) that test_pose_ransac_cpu.py shows the case to tell apart."""
    lc = list_chunks(cameras, n_usable)
    part, out = np.zeros(lc[-1] + len(cameras), np.int64), np.zeros(len(cameras), np.int64)
    for c0 in range(0, len(cameras), tile):
        c1 = min(c0 + tile, len(cameras))
        at = lc[c0] if offset == "chunk" else c0
        for c in range(c0, c1):
            m = masks[cameras[c]]
            for j in range(lc[c + 1] - lc[c]):
                part[at + (lc[c] - lc[c0]) + j] = m[CHUNK * j: CHUNK * (j + 1)].sum()
        for c in range(c0, c1):
            out[c] = part[lc[c]: lc[c + 1]].sum()
    return out


@functools.lru_cache(maxsize=None)
def bootstrap_case(frac=BOOT_FRACTION):
    """"300x8" with ``frac`` of the observations of cameras 2 .. 7 replaced by uniform positions: (scene, xy', replaced)."""
    sc = IC.tri_scene("300x8")
    xy, hit = contaminate(sc.cam_idx, sc.xy, frac, cameras=np.arange(2, 8))
    for a in (xy, hit):
        a.setflags(write=False)
    return sc, xy, hit


@functools.lru_cache(maxsize=None)
def reference_bootstrap(linear="eigh"):
    from lib.initialization import engine_intrinsics

    sc, xy, _ = bootstrap_case()
    return QR.bootstrap(sc.pt_ptr, sc.cam_idx, xy, engine_intrinsics(sc.init_K), THRESHOLD, 512, 1, start_pair=(0, 1), max_rms=0.01, linear=linear)


@functools.lru_cache(maxsize=None)
def plain_bootstrap(contaminated):
    """tests/_twoview_ref.py's bootstrap (plain resection) on the clean or on the contaminated tracks; None if it raises."""
    from lib.initialization import engine_intrinsics

    sc, xy, _ = bootstrap_case()
    try:
        return T.bootstrap(sc.pt_ptr, sc.cam_idx, xy if contaminated else sc.xy, engine_intrinsics(sc.init_K), start_pair=(0, 1), max_rms=0.01)
    except ValueError:
        return None


def true_poses(sc):
    """The ground-truth poses in bootstrap's output frame: camera 0 at the origin with identity pose, |t_1 - t_0| = 1."""
    R0, t0, s = sc.R_gt[0], sc.t_gt[0], np.linalg.norm(sc.t_gt[1] - sc.t_gt[0])
    return R0.T @ sc.R_gt, ((sc.t_gt - t0) @ R0) / s


def pose_error(sc, R, t, camera_ok):
    """(max abs error of R, of t) over the registered cameras against the ground truth."""
    Rg, tg = true_poses(sc)
    return np.abs(R[camera_ok] - Rg[camera_ok]).max(), np.abs(t[camera_ok] - tg[camera_ok]).max()
