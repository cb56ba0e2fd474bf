"""Structured visibility families for the bundle-adjustment tests (test_visibility_cases_cpu.py proves their regimes on the
host), each built once.  A case is a fully visible make_scene (host projections: no device needed) under a
deterministic boolean (n, m) keep-mask, so geometry, noise and initial estimates stay make_scene's and only WHO SEES WHAT
changes.  Every family is tied to one part of csrc/mvba_create.h that iid visibility leaves unexercised; the sizing formulas
of that file are restated here in NumPy so that a CPU test can prove the regime is reached.  Test infrastructure only."""
import functools

import numpy as np

from lib.synthetic import make_scene

SEED = 7
BAND_W = 4
# csrc/mvba_create.h
SLOT_SKEW = 12288
SLOT_SEG = 8192   # pacing segment of the slot form, in observations
PSTEP = 21       # lists per wave of the slot form
S_CAP = 256      # sub-lists per pair at most


# ---------------------------------------------------------------- the keep-masks
def band_mask(n, m, w=BAND_W, w_min=2, seed=SEED):
    """Sequential capture: point a is seen by cameras [s_a, s_a + w_a), s_a = a (m - w + 1) // n, w_a in {w_min .. w}.
    Reaches: most camera pairs empty, every list confined to a stretch of the point sweep, queues and waves of unequal length."""
    a = np.arange(n)
    s = a * (m - w + 1) // n
    wa = np.random.default_rng(seed).integers(w_min, w + 1, n)
    k = np.arange(m)[None, :]
    return (k >= s[:, None]) & (k < (s + wa)[:, None])


def hub_mask(n, m, n_full=8, seed=SEED):
    """Camera 0 sees every point, every point has one more camera drawn uniformly, n_full evenly spaced points are seen by all.
    Reaches: the cap of 256 sub-lists on camera 0's diagonal pair, a typical pair of a few dozen items, point degree 2 beside
    m, camera degree n beside ~n / m."""
    keep = np.zeros((n, m), bool)
    keep[:, 0] = True
    keep[np.arange(n), np.random.default_rng(seed).integers(1, m, n)] = True
    keep[(2 * np.arange(n_full) + 1) * n // (2 * n_full)] = True
    return keep


def blocks_mask(n, m, n_bridge=20, p=0.5, seed=SEED):
    """Two clusters: cameras [0, m/2) see only the first half of the points (each with probability p), the others only the
    second half; the n_bridge points around n / 2 are seen by all; a point left with fewer than 2 views gets views inside its
    block.  Reaches: lists and whole waves absent from half the point ranges."""
    rng = np.random.default_rng(seed)
    keep = rng.random((n, m)) < p
    first = np.arange(n) < n // 2
    left = np.arange(m) < m // 2
    keep &= first[:, None] == left[None, :]
    for a in np.nonzero(keep.sum(1) < 2)[0]:
        cams = np.arange(m // 2) if first[a] else np.arange(m // 2, m)
        keep[a, rng.choice(cams, size=2, replace=False)] = True
    keep[n // 2 - n_bridge // 2:n // 2 + (n_bridge + 1) // 2] = True
    return keep


def heavy_mask(n, m):
    """Every point is seen by two neighbouring cameras k, k + 1 (k sweeps the cameras with the points); the points n/5, n/2 and
    n - 1 are seen by all m.  With few enough points one heavy point carries more items than a point range's share: ranges
    without a single point."""
    keep = np.zeros((n, m), bool)
    k = np.arange(n) * (m - 1) // n
    keep[np.arange(n), k] = keep[np.arange(n), k + 1] = True
    keep[[n // 5, n // 2, n - 1]] = True
    return keep


# ---------------------------------------------------------------- the cases
CASES = {  # name: (n, m, mask)
    "band_3000x14": (3000, 14, band_mask),
    "band_30000x24": (30000, 24, band_mask),
    "hub_20000x40": (20000, 40, hub_mask),
    "blocks_20000x20": (20000, 20, blocks_mask),
    "heavy_1500x60": (1500, 60, heavy_mask),
    # skew idling: ranges of the slot form wider than 2 x SLOT_SKEW observations
    "band_150000x34": (150000, 34, band_mask),
}
SKEW_CASE = "band_150000x34"
TABLE = ("band_3000x14", "band_30000x24", "hub_20000x40", "blocks_20000x20", "heavy_1500x60")


def masked(sc, keep):
    """(pt_ptr, cam_idx, xy) of the fully visible scene `sc` under the (n, m) keep-mask."""
    n, m = keep.shape
    assert sc.n_obs == n * m
    pt_ptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    cam_idx = np.nonzero(keep)[1].astype(np.int32)
    return pt_ptr, cam_idx, np.ascontiguousarray(sc.xy.reshape(n, m, 2)[keep])


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, pt_ptr, cam_idx, xy): the scene is make_scene's full-visibility one (its own pt_ptr / cam_idx / xy are NOT the
    case's), the other three are the case's observation list."""
    n, m, mask = CASES[name]
    sc = make_scene(n, m, vis_p=1.0, project="numpy")
    out = (sc,) + masked(sc, mask(n, m))
    for a in out[1:]:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- csrc/mvba_create.h, restated
def pair_counts(pt_ptr, cam_idx, m):
    """(m, m) int64, upper triangle: items of every camera pair k <= l (the diagonal: camera k's observations)."""
    deg = np.diff(pt_ptr)
    cnt = np.zeros((m, m), np.int64)
    for d in np.unique(deg):
        rows = cam_idx[(pt_ptr[:-1][deg == d][:, None] + np.arange(d)[None, :])]  # (points of degree d, d), ascending
        i, j = np.triu_indices(d)
        np.add.at(cnt, (rows[:, i].ravel(), rows[:, j].ravel()), 1)
    return cnt


def size_pair_lists(cnt):
    """size_pair_lists: (target, S (m, m) upper triangle, slot_waves)."""
    m = cnt.shape[0]
    iu = np.triu_indices(m)
    off = np.triu_indices(m, 1)
    T, Tdiag, P = int(cnt[iu].sum()), int(np.trace(cnt)), m * (m + 1) // 2
    target = max(1, (T - Tdiag) // max(1, P - m))
    S = np.zeros_like(cnt)
    S[iu] = np.clip((cnt[iu] + target // 2) // target, 1, S_CAP)
    slot_waves = -(-int(np.trace(S)) // PSTEP) + -(-int(S[off].sum()) // PSTEP)
    return target, S, slot_waves


def slot_ranges(pt_ptr, target, slot_waves, xcd_waves=32 * 9):
    """make_ranges, slot branch: first point of every range, [nR + 1].  xcd_waves = CUs / 8 x 9 waves per CU: 288 on the
    MI355X's 256 CUs.  It enters through min(xcd_waves // slot_waves, target // 512) only: every case here but blocks has
    target < 1024 (nR = 8 on any device) and blocks has 18 waves per range (nR = 16 from 36 waves per XCD up)."""
    j = max(1, min(xcd_waves // max(1, slot_waves), target // 512))
    nR = 8 * min(j, 8)
    d = np.diff(pt_ptr)
    pre = np.concatenate([[0], np.cumsum(d * (d + 1) // 2)])
    lo = np.searchsorted(pre, [int(pre[-1]) * r // nR for r in range(nR + 1)], side="left")
    lo[0], lo[nR] = 0, len(d)
    return lo


def first_points(pt_ptr, cam_idx, m):
    """(m, m) upper triangle: the first (lowest) point of every camera pair's list, -1 for an empty pair."""
    n = len(pt_ptr) - 1
    deg = np.diff(pt_ptr)
    first = np.full((m, m), n, np.int64)
    pts = np.arange(n)
    for d in np.unique(deg):
        sel = pts[deg == d]
        rows = cam_idx[(pt_ptr[:-1][sel][:, None] + np.arange(d)[None, :])]
        i, j = np.triu_indices(d)
        np.minimum.at(first, (rows[:, i].ravel(), rows[:, j].ravel()), np.repeat(sel, len(i)))
    first[first == n] = -1
    return first


def skew_precondition(pt_ptr, cam_idx, m):
    """From the observation list alone: the slot plan has 8 point ranges, each wider than 2 x SLOT_SKEW observations, and
    inside one of them two non-empty pairs (k, l), (k, l + 1) whose first items IN THAT RANGE lie more than SLOT_SKEW
    observations apart -- the later list's slot idles while the earlier one runs.  A proxy for two slots of one wave: the
    lists of a wave are 21 consecutive (pair, sub-list) entries in (k, l) order, so the last sub-list of (k, l) and the first
    of (k, l + 1) are neighbours and share a wave unless a wave boundary falls between them; a pair's sub-lists are dealt
    round-robin and start within S items of each other."""
    target, _, slot_waves = size_pair_lists(pair_counts(pt_ptr, cam_idx, m))
    lo = slot_ranges(pt_ptr, target, slot_waves)
    if len(lo) != 9 or np.diff(pt_ptr[lo]).min() <= 2 * SLOT_SKEW:
        return False
    for r in range(8):
        o0, o1 = pt_ptr[lo[r]], pt_ptr[lo[r + 1]]
        sub_ptr = pt_ptr[lo[r]:lo[r + 1] + 1] - o0
        first = first_points(sub_ptr, cam_idx[o0:o1], m)  # (points counted from the range's first)
        for k in range(m):
            for l in range(k + 1, m - 1):  # (off-diagonal: the diagonal pairs' lists go into waves of their own)
                a, b = first[k, l], first[k, l + 1]
                if a >= 0 and b >= 0 and abs(int(sub_ptr[b]) - int(sub_ptr[a])) > SLOT_SKEW:
                    return True
    return False


def oracle_for(name):
    """The CPU oracle at the case's initial estimates (normalised frame), not yet linearised."""
    from oracle import ba_oracle as O

    sc, pt_ptr, cam_idx, xy = case(name)
    g = O.OracleEngine(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, 1.0, sc.axis)
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    g.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    return g
