"""Visibility families for the code the engine picks by a point's DEGREE (the number of cameras that see it), in the style of
tests/_visibility_cases.py (test_degree_cases_cpu.py proves their regimes on the host), each built once.
  tall  a few points seen by 64 .. 300 cameras in a sea of band points of degree 2 .. 5: K1's split tiles beside packed ones,
        and the kernels that are sized by the MEAN degree (K5 at two lanes per point, k_point_cov at eight) on an outlier
  wide  iid visibility with a mean degree above 40 and above 100 at every block size of K5
The selection rules of csrc/mvba.hip (the launch side; the kernels are in csrc/mvba_linearize.h and csrc/mvba_tail.h) and
csrc/mvba_create.h are restated here in NumPy.  Test infrastructure only."""
import functools

import numpy as np

import _visibility_cases as V
from lib.bundle_adjustment import to_gauge_frame
from lib.synthetic import make_scene
from oracle import ba_oracle as O

SEED = 7


# ---------------------------------------------------------------- the keep-masks
def tall_mask(n, m, tall, w=V.BAND_W, w_min=2):
    """band_mask(n, m, w, w_min) with the rows of the points in `tall` ({point: degree}) replaced by "seen by cameras
    0 .. degree - 1"."""
    keep = V.band_mask(n, m, w, w_min)
    k = np.arange(m)
    for a, d in tall.items():
        keep[a] = k < d
    return keep


def wide_mask(n, m, p, seed=SEED):
    return np.random.default_rng(seed).random((n, m)) < p


# ---------------------------------------------------------------- the cases
# Point 0 tall: the first tile is a split one (~0 = -1).  The last point tall: the terminator follows a split tile.  Points 1 .. 6
# part-fill a packed tile, point 7 (exactly 64) fills a packed tile alone, points 8 and 9 are two split points in a row.
# Degrees 65, 129, 193 and 257 end in a piece of one observation, 128 in a full piece; 2, 3, 4 and 5 pieces occur.
TALL = {  # name: (n, m, {point: degree}, band w, band w_min)
    # w = 5: with the band at degrees 2 .. 4 the two covariance references agree to 1.2e-10 only (COV_REF_DIFF below wants 1e-10)
    "tall_1500x80": (1500, 80, {0: 65, 7: 64, 8: 80, 9: 79, 750: 80, 1499: 66}, 5, 2),
    "tall_2000x130": (2000, 130, {0: 65, 7: 64, 8: 129, 9: 128, 1000: 130, 1001: 127, 1999: 66}, 4, 2),
    # w_min = 3: with degrees 2 .. 4 the band leaves camera 299 with 3 observations, and the undamped covariance wants 5
    "tall_6000x300": (6000, 300, {0: 65, 7: 64, 8: 129, 9: 128, 3000: 300, 3001: 193, 5999: 257}, 4, 3),
}
# 60 points where that leaves every camera MIN_CAMERA_DEGREE observations; more where it does not (with 60 points the draw of
# 400 x 0.2 leaves a camera with 4, of 647 x 0.2 with 3, of 647 x 0.1 with 1).  The mean degree m p does not depend on n.
WIDE = {  # name: (n, m, p); the K5 cell of each: K5_CELL below
    "wide_40x110": (40, 110, 1.0),
    "wide_60x200_60": (60, 200, 0.6),
    "wide_60x400_35": (60, 400, 0.35),
    "wide_80x647_20": (80, 647, 0.2),
    "wide_60x200_35": (60, 200, 0.35),
    "wide_80x400_20": (80, 400, 0.2),
    "wide_200x647_10": (200, 647, 0.1),  # 85 of its 200 points are split: a second mixed tile layout
}
CASES = tuple(TALL) + tuple(WIDE)
# iid scenes for the robust twins alone (ROBUST_CASES below), kept out of CASES: the robust (G, bt) cells of k_backsub that no
# case above reaches with a Huber twin inside ROBUST_SELF_DIFF_BOUND (tall_6000x300 gives 1.12e-11, wide_80x400_20 1.04e-11)
ROBUST_WIDE = {  # name: (n, m, p); point degrees, fewest observations of a camera
    "wide_60x90_60": (60, 90, 0.6),     # 43 .. 65, 26
    "wide_300x200_10": (300, 200, 0.1),  # 8 .. 33, 19
    "wide_300x400_05": (300, 400, 0.05),  # 10 .. 34, 5
    "wide_120x400_15": (120, 400, 0.15),  # 41 .. 77, 7
}
MIN_CAMERA_DEGREE = 5  # the undamped reduced system (covariance) wants a few observations per camera


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, pt_ptr, cam_idx, xy) as tests/_visibility_cases.py::case: the scene is make_scene's fully visible one, the other
    three are the case's observation list, read-only."""
    if name in TALL:
        n, m, tall, w, w_min = TALL[name]
        keep = tall_mask(n, m, tall, w, w_min)
    else:
        n, m, p = WIDE[name] if name in WIDE else ROBUST_WIDE[name]
        keep = wide_mask(n, m, p)
    sc = make_scene(n, m, vis_p=1.0, project="numpy")
    out = (sc,) + V.masked(sc, keep)
    for a in out[1:]:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- csrc/mvba_create.h::build_k1_tiles, restated
def k1_tiles(pt_ptr):
    """(tiles, tile_slot, splits): the tile starts with the terminator n_obs at the end, a split tile's start complemented
    (~start < 0); tile_slot as it is uploaded ([len(tiles)], -1 where a tile is no piece); splits = rows (point, first slot,
    pieces)."""
    tiles, slot_of, splits = [], {}, []
    cur0 = fill = n_slots = 0
    d_all = np.diff(pt_ptr)
    for a, d in enumerate(d_all.tolist()):
        if d > 64:
            if fill:
                tiles.append(cur0)
                cur0, fill = cur0 + fill, 0
            splits.append((a, n_slots, (d + 63) // 64))
            for q in range(0, d, 64):
                slot_of[len(tiles)] = n_slots
                n_slots += 1
                tiles.append(~cur0)
                cur0 += min(64, d - q)
            continue
        if fill + d > 64:
            tiles.append(cur0)
            cur0, fill = cur0 + fill, 0
        fill += d
    if fill:
        tiles.append(cur0)
        cur0 += fill
    assert cur0 == pt_ptr[-1]
    tiles.append(int(pt_ptr[-1]))
    tile_slot = np.full(len(tiles), -1, np.int64)
    for t, s in slot_of.items():
        tile_slot[t] = s
    return np.array(tiles, np.int64), tile_slot, np.array(splits, np.int64).reshape(-1, 3)


def tile_ranges(tiles):
    """(first observation, one past the last, split flag) of every tile, as k_resid_jac decodes tile_start."""
    start = np.where(tiles < 0, ~tiles, tiles)
    return start[:-1], start[1:], tiles[:-1] < 0


# ---------------------------------------------------------------- csrc/mvba_engine_host.h (k5_lanes, table_block_threads, cov_lanes;
# launched by launch_tail_and_cost in csrc/mvba_step.h and cov_blocks in csrc/mvba_cov_host.h; LDS_CAMERAS: csrc/mvba_device.h): the
# width rules, restated
CAM_LDS, DXI_LDS, LDS_CAMERAS = 18, 10, 646
K5_G_LIMITS = (40.0, 100.0)       # mean degree: two lanes per point up to 40, four up to 100, eight beyond
COV_G_LIMITS = (12.0, 24.0, 48.0)  # mean pair count 0.5 d (d + 1): 8 lanes up to 12, 16 up to 24, 32 up to 48, 64 beyond
GCAM = "gcam"


def k5_cell(n_obs, n, m, g_limits=K5_G_LIMITS):
    """launch_tail_and_cost: (G, bt) of k_backsub; bt is GCAM once the camera tables are in device memory."""
    deg = n_obs / n
    G = 2 if deg <= g_limits[0] else (4 if deg <= g_limits[1] else 8)
    if m > LDS_CAMERAS:
        return G, GCAM
    lds = m * (CAM_LDS + DXI_LDS) * 8
    return G, 1024 if lds > 80 * 1024 else (512 if lds > 40 * 1024 else 256)


def cov_lanes(n_obs, n):
    """mvba_covariance: lanes per point of k_point_cov."""
    d = n_obs / n
    pairs = 0.5 * d * (d + 1.0)
    return 64 if pairs > COV_G_LIMITS[2] else (32 if pairs > COV_G_LIMITS[1] else (16 if pairs > COV_G_LIMITS[0] else 8))


K5_CELL = {  # what every case must reach (test_degree_cases_cpu.py asserts it from the observation list)
    "tall_1500x80": (2, 256), "tall_2000x130": (2, 256), "tall_6000x300": (2, 512),
    "wide_40x110": (8, 256), "wide_60x200_60": (8, 512), "wide_60x400_35": (8, 1024), "wide_80x647_20": (8, GCAM),
    "wide_60x200_35": (4, 512), "wide_80x400_20": (4, 1024), "wide_200x647_10": (4, GCAM),
}
ROBUST_WIDE_K5_CELL = {"wide_60x90_60": (4, 256), "wide_300x200_10": (2, 512), "wide_300x400_05": (2, 1024), "wide_120x400_15": (4, 1024)}
ALL_K5_CELLS = {(G, bt) for G in (2, 4, 8) for bt in (256, 512, 1024, GCAM)}
# The iid scenes (n, m, vis_p) of tests/test_gpu_parity.py that reach the cells these families do not: (90, 70, 1.0) is the
# only one with four lanes, the two of test_extreme_camera_counts_vs_oracle have two lanes at 1024 threads and with GCAM
# (their mean degree is m vis_p = 26: the draw cannot move it across 40).
OLD_K5_SCENES = ((90, 70, 1.0), (3000, 646, 0.04), (3000, 647, 0.04))


# ---------------------------------------------------------------- the oracle, once per case
class CachedOracle(O.OracleEngine):
    """An OracleEngine whose linearisation and reduced systems are computed once per damping: it is never committed, so every
    test that reads it sees the case's initial state.  (Linearise + one trial of a 647-camera case takes the host a quarter of
    a minute, and tests/_parity_checks.py::check_one_step asks for the reduced system twice.)"""
    _lin = False

    def linearize(self):
        if not self._lin:
            super().linearize()
            self._lin, self._sys = True, {}

    def reduced_system(self, c):
        if c not in self._sys:
            A, b = super().reduced_system(c)
            A.setflags(write=False), b.setflags(write=False)
            self._sys[c] = (A, b, self.Einv)
        A, b, self.Einv = self._sys[c]
        return A, b

    def commit(self):
        raise RuntimeError("shared between tests: never committed")


@functools.lru_cache(maxsize=None)
def oracle_for(name):
    """The shared oracle of a case at its initial estimates (normalised frame), not yet linearised."""
    sc, pt_ptr, cam_idx, xy = case(name)
    g = CachedOracle(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, 1.0, sc.axis)
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    g.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    return g


def problem(name, xy=None):
    """The case as the tuple tests/test_gpu_covariance.py and tests/test_gpu_robust.py pass around."""
    sc, pt_ptr, cam_idx, xy0 = case(name)
    X, R, t = to_gauge_frame(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    return (sc.n_points, sc.n_images, pt_ptr, cam_idx, xy0 if xy is None else xy, 1.0, sc.axis, X, sc.init_K[:, 0, 0],
            sc.init_K[:, :2, 2], t, R)


# Every robust (G, bt) cell of k_backsub but (2, 256) and (2, GCAM), which tests/test_gpu_robust.py runs: K5_CELL and
# ROBUST_WIDE_K5_CELL name the cell of each.
ROBUST_CASES = ("tall_2000x130", "wide_40x110", "wide_80x647_20", "wide_60x200_35", "wide_60x200_60", "wide_60x400_35",
                "wide_200x647_10") + tuple(ROBUST_WIDE)
ROBUST_LOSSES = (("huber", 3.0), ("cauchy", 2.0))


@functools.lru_cache(maxsize=None)
def outlier_xy(name):
    """The case's observations with the gross outliers of tests/test_gpu_robust.py::_scene."""
    from _robust_ref import inject_outliers

    xy, _ = inject_outliers(np.array(case(name)[3]), 0.08, 20.0, 100.0, seed=5)
    xy.setflags(write=False)
    return xy


def reversed_inside_points(pt_ptr, *per_obs):
    """The per-observation arrays with the order reversed inside every point: the same problem to an oracle (which does not
    ask for ascending cameras), every per-point and per-camera sum taken in another order."""
    idx = np.concatenate([np.arange(pt_ptr[a + 1] - 1, pt_ptr[a] - 1, -1) for a in range(len(pt_ptr) - 1)])
    return tuple(np.ascontiguousarray(v[idx]) for v in per_obs)


# ---------------------------------------------------------------- figures measured on the host (test_degree_cases_cpu.py)
# The robust twins run at damping 1e-2, not at tests/test_gpu_robust.py::_check_step's default 1e-3.  The outliers are 20 .. 100
# units in an image of size ~1, and with Huber's unbounded influence the first trial is no descent step: at 1e-3 the camera
# update of wide_80x647_20 reaches 139 (radians, among others), the trial cost is 14 x the cost it started from, and the
# ORACLE's trial cost differs from its own by 7.2e-10 relative when the sums inside every point are taken in reversed order --
# at _check_step's bound of 1e-9, with dX equal to 3e-14.  At 1e-2 the same figure is 7.4e-12 (tall_2000x130 3.9e-12,
# wide_40x110 5.6e-13, wide_60x200_35 6.7e-14, wide_60x200_60 2.9e-15, wide_60x400_35 3.8e-13, wide_200x647_10 3.7e-12,
# wide_60x90_60 5.0e-12, wide_300x200_10 2.5e-13, wide_300x400_05 1.0e-12, wide_120x400_15 6.4e-14, every Cauchy twin below
# 1e-15): 100 x below the bound, which test_degree_cases_cpu.py asserts for every twin.
ROBUST_C = 1e-2
ROBUST_SELF_DIFF_BOUND = 1e-11
MARGIN = 100.0  # a GPU assert gets MARGIN x the host-versus-host figure of its case (tests/_init_cases.py)
# tall_1500x80, reference against reference: tests/_covariance_ref.py::schur_covariance against dense_covariance, max abs
# difference over the largest entry.  The GPU is held to schur_covariance at 1e-8 (tests/test_gpu_covariance.py::_check).
COV_REF_DIFF = {"points": 4.8e-11, "cameras": 5.7e-11, "cameras_full": 6.2e-11}
# tall_6000x300: eigh of the moment matrix against the SVD of the stacked rows, max |dX| of the linear step (points of order 1)
TRI_HOST_DIFF = 1.3e-13


def tri_args(name):
    """(K, R, t, pt_ptr, cam_idx, xy) of a case as BundleAdjuster.from_observations(init_X=None) hands them to the engine:
    the initial cameras in the gauge frame."""
    sc, pt_ptr, cam_idx, xy = case(name)
    _, R, t = to_gauge_frame(np.zeros((0, 3)), sc.init_R, sc.init_t, sc.axis)
    return sc.init_K, R, t, pt_ptr, cam_idx, xy


@functools.lru_cache(maxsize=None)
def tri_reference(name="tall_6000x300"):
    """tests/_init_ref.py::triangulate with the two refinement steps of init_X=None."""
    import _init_ref as ref

    out = ref.triangulate(*tri_args(name), 2)
    for v in out:
        v.setflags(write=False)
    return out
