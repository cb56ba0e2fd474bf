"""Inputs shared by test_tracks_cpu.py and test_gpu_tracks.py, each built once: the hand-made match graphs of DESIGN.md §24
(their premises are asserted here, where they are defined), the helper that turns an observation list into what a matcher
would deliver, and the scenes built with it.  Test infrastructure only."""
import functools
from types import SimpleNamespace

import numpy as np

import _tracks_ref as TR

LANE_MAX = 32  # csrc/mvba_tracks.h: TRK_LANE_MAX, the entries up to which one lane sorts a track
BLOCK = 256    # threads per workgroup of every kernel there


def _graph(counts, edges, edge_ok=None, min_length=2):
    """(kp_ptr, kp_xy, edges, edge_ok, min_length) with kp_xy made of the node id, so that a copy is recognised."""
    kp_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(kp_ptr[-1])
    kp_xy = np.stack([np.arange(n) + 0.25, -np.arange(n) - 0.5], axis=1)
    edges = np.asarray(edges, np.int32).reshape(-1, 2)
    assert n == 0 or len(edges) == 0 or (0 <= edges.min() and edges.max() < n)
    out = kp_ptr, kp_xy, edges, None if edge_ok is None else np.asarray(edge_ok, np.uint8), min_length
    for a in out[:4]:
        if a is not None:
            a.setflags(write=False)
    return out


def _tiny():
    """The smallest conflict: a0, b0 in image 0 both matched to c1 in image 1; beside it a clean track d0 - e1 - f2."""
    a0, b0, d0, c1, e1, f2 = range(6)
    return _graph([3, 2, 1], [(a0, c1), (b0, c1), (d0, e1), (e1, f2)])


def _blocks():
    """257 tracks x 3 images, one more than a workgroup has threads: track i is nodes i, 257 + i, 514 + i, and edge 255 | 256 of
    the list, like nodes 255 | 256, lie on either side of a workgroup boundary."""
    n = BLOCK + 1
    i = np.arange(n)
    return _graph([n, n, n], np.concatenate([np.stack([i, n + i], axis=1), np.stack([2 * n + i, n + i], axis=1)]))


def _path(m, extra_in_image_0):
    """m images; one keypoint each makes a path through all of them, its edges (i, i + 1) listed from the far end.  With
    ``extra_in_image_0`` image 0 has a second keypoint tied to the far end.  Beside the path, second keypoints of images 1, 2, 3
    form a clean track."""
    counts = np.ones(m, np.int64)
    counts[1:4] += 1
    counts[0] += bool(extra_in_image_0)
    kp_ptr = np.concatenate([[0], np.cumsum(counts)])
    first = kp_ptr[:-1] + (np.arange(m) == 0) * bool(extra_in_image_0)  # (image 0's path keypoint comes after its extra one)
    edges = [(first[i], first[i + 1]) for i in range(m - 1)][::-1]
    if extra_in_image_0:
        edges.append((first[m - 1], 0))
    side = kp_ptr[1:4] + 1
    edges += [(side[0], side[1]), (side[2], side[1])]
    g = _graph(counts, edges)
    size = np.bincount(TR.labels(int(kp_ptr[-1]), g[2]))
    assert sorted(size[size > 0].tolist()) == [3, m + bool(extra_in_image_0)]  # exactly n_images nodes, or exactly one more
    return g


def _sort32():
    """70 images; five tracks of 31, 32, 33, 64 and 65 keypoints -- on both sides of the lane / wave boundary of the segment sort, and
    of a wave's 64 lanes --, each over a random set of images, joined by a random spanning tree whose edges come in random order."""
    rng = np.random.default_rng(32)
    m, lengths = 70, (LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, 64, 65)
    images = [np.sort(rng.choice(m, L, replace=False)) for L in lengths]
    counts = np.bincount(np.concatenate(images), minlength=m)
    kp_ptr = np.concatenate([[0], np.cumsum(counts)])
    used = np.zeros(m, np.int64)
    edges = []
    for im in images:
        nodes = kp_ptr[im] + used[im]
        used[im] += 1
        nodes = rng.permutation(nodes)
        edges += [(nodes[i], nodes[rng.integers(i)]) for i in range(1, len(nodes))]
    g = _graph(counts, rng.permutation(np.array(edges), axis=0))
    size = np.bincount(TR.labels(int(kp_ptr[-1]), g[2]))
    assert sorted(size[size > 0].tolist()) == sorted(lengths) and max(lengths) <= m
    return g


def _hub():
    """5000 keypoints, 100 in each of images 1 .. 50, all matched to node 0 of image 0: every thread of the first round hits one
    word.  5001 nodes > 51 images: oversize.  Beside it a clean pair in images 1 and 2."""
    counts = np.array([1] + [101, 101] + [100] * 48)
    kp_ptr = np.concatenate([[0], np.cumsum(counts)])
    spokes = np.concatenate([kp_ptr[i] + np.arange(100) for i in range(1, 51)])
    edges = [(0, s) if s % 2 else (s, 0) for s in spokes] + [(kp_ptr[1] + 100, kp_ptr[2] + 100)]
    g = _graph(counts, edges)
    size = np.bincount(TR.labels(int(kp_ptr[-1]), g[2]))
    assert sorted(size[size > 0].tolist()) == [2, 5001] and 5001 > len(counts)
    return g


def _messy():
    """Images 0 .. 4 with 3, 3, 0, 3, 2 keypoints (image 2 has none), min_length = 3.  A = {0, 3, 6}: a clean track whose first
    edge comes three times, once turned round; the masked-out edge (0, 1) would put a second keypoint of image 0 into it.  (1, 1)
    and (5, 5) are loops: 1, 5 and the untouched 10 are unmatched.  {2, 7, 8} holds the same-image edge (7, 8): conflicting.  {4, 9}
    is a pair, shorter than min_length."""
    edges = [(0, 3), (3, 0), (0, 3), (0, 1), (3, 6), (1, 1), (5, 5), (2, 7), (7, 8), (9, 4)]
    ok = [e != (0, 1) for e in edges]
    return _graph([3, 3, 0, 3, 2], edges, ok, 3)


def _empty():
    return _graph([0], np.zeros((0, 2), np.int32))


def _path4096():
    """4096 images with one keypoint each, the path's edges in a seeded random order, half of them turned round."""
    rng = np.random.default_rng(4096)
    e = np.stack([np.arange(4095), np.arange(1, 4096)], axis=1)
    flip = rng.random(4095) < 0.5
    e[flip] = e[flip][:, ::-1]
    return _graph(np.ones(4096, np.int64), rng.permutation(e, axis=0))


GRAPHS = {"tiny": _tiny, "blocks": _blocks, "path130": lambda: _path(130, False), "path131": lambda: _path(130, True), "sort32": _sort32,
          "hub": _hub, "messy": _messy, "empty": _empty, "path4096": _path4096}
# node_track of the hand-made cases small enough to state
NODE_TRACK = {"tiny": [-3, -3, 0, -3, 0, 0], "messy": [0, -1, -3, 0, -2, -1, 0, -3, -3, -2, -1]}


@functools.lru_cache(maxsize=None)
def graph(name):
    return GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    kp_ptr, kp_xy, edges, ok, min_length = graph(name)
    return TR.build_tracks(kp_ptr, kp_xy, edges, ok, min_length)


# ---- the structural limits of the kernels ("Limits pass") ---------------------------------------------------
# Graphs of their own, beside GRAPHS.
SCAN_BLOCK = 1024        # csrc/mvba_tracks.h: TRK_SCAN_BLOCK, the nodes of a block of the scan
SCAN_SUMS = 256          # block totals k_tracks_scan_sums takes per trip: the second trip starts at node 262 144
HOOK_EDGES = 8192 * 256  # TRK_HOOK_GRID workgroups of 256 threads: the grid stride of k_tracks_hook starts beyond
BIG_M, BIG_T = 87_400, 1_100  # keypoints of images 0 .. 2 and of images 3 .. 5: the small images lie beyond node 262 144
BIG_COPIES = 16          # the long form lists every edge this often, and once more turned round


def _big_part(base, m, period):
    """Tracks i = 0 .. m - 1 over three images of m keypoints from node ``base`` on: a = base + i, b = a + m, c = b + m.  By
    k = i mod period: 7 -- a - b - c and b - (a + 1): two keypoints of one image, a conflict of 4 nodes; 8 -- no edge of its
    own (its a is in the conflict before it, its b and c stay unmatched); 20 -- a - b alone, shorter than min_length = 3, c
    unmatched; 30, 31, 32 -- three tracks chained c - (a + 1): 9 nodes, more than the 6 images; every other k -- the clean
    track a - b - c."""
    i = np.arange(m)
    k = i % period
    a, b, c = base + i, base + m + i, base + 2 * m + i
    full = (k != 8) & (k != 20)
    e = [np.stack([a[full], b[full]], axis=1), np.stack([c[full], b[full]], axis=1), np.stack([b[k == 20], a[k == 20]], axis=1),
         np.stack([b[k == 7], a[k == 7] + 1], axis=1), np.stack([c[(k == 30) | (k == 31)], a[(k == 30) | (k == 31)] + 1], axis=1)]
    assert i[k == 7].max() + 1 < m and i[k == 31].max() + 1 < m
    return np.concatenate(e)


@functools.lru_cache(maxsize=None)
def _big_edges():
    rng = np.random.default_rng(260)
    e = np.concatenate([_big_part(0, BIG_M, 1000), _big_part(3 * BIG_M, BIG_T, 100)])
    return rng.permutation(e, axis=0)


def _big(long):
    """Images of BIG_M, BIG_M, BIG_M, BIG_T, BIG_T, BIG_T keypoints: 265 500 nodes, 260 scan blocks, with _big_part's tracks over
    the first three and over the last three (whose roots lie in scan blocks 256 and 257), min_length = 3.  ``long``: every edge
    BIG_COPIES times and once turned round, in a random order -- more edges than one sweep of the hook kernel's grid takes."""
    e = _big_edges()
    if long:
        e = np.random.default_rng(261).permutation(np.concatenate([e] * BIG_COPIES + [e[:, ::-1]]), axis=0)
    return _graph([BIG_M] * 3 + [BIG_T] * 3, e, None, 3)


SORT_M, SORT_N = 70, 300
# candidate rank -> length: lanes 0, 62, 63 of wave 0; lanes 0, 1, 63 of wave 1; lane 0 of wave 2; lanes 8, 63 of wave 3; and
# lanes 0 and 43 of the second workgroup.  (The last long track is the longest: whatever length a lane applies to the wrong
# segment, it stays inside the buffer.)
SORT_LONG = {0: 33, 62: 40, 63: 64, 64: 65, 65: 70, 127: 33, 128: 40, 200: 64, 255: 65, 256: 40, 299: 70}


def _sort_waves():
    """SORT_M images; image 0 has SORT_N keypoints and track c starts at its keypoint c, so candidate c IS track c.  The tracks
    of SORT_LONG have 33 .. 70 keypoints, all others 2 or 3; each over a random set of images, joined by a random spanning tree,
    the edges of all of them in one random order."""
    rng = np.random.default_rng(300)
    lengths = [SORT_LONG.get(c, 2 + int(rng.integers(2))) for c in range(SORT_N)]
    images = [np.concatenate([[0], 1 + np.sort(rng.choice(SORT_M - 1, L - 1, replace=False))]) for L in lengths]
    counts = np.bincount(np.concatenate(images), minlength=SORT_M)
    kp_ptr = np.concatenate([[0], np.cumsum(counts)])
    used = np.zeros(SORT_M, np.int64)
    edges = []
    for im in images:
        nodes = kp_ptr[im] + used[im]
        used[im] += 1
        nodes = rng.permutation(nodes)
        edges += [(nodes[i], nodes[rng.integers(i)]) for i in range(1, len(nodes))]
    assert counts[0] == SORT_N and max(lengths) <= SORT_M
    return _graph(counts, rng.permutation(np.array(edges), axis=0))


def _ends():
    """Images 0 .. 7 with 0, 2, 2, 0, 0, 2, 1, 0 keypoints: the first and the last image are empty, and two in the middle in a row.
    Tracks {0, 2, 4} (images 1, 2, 5) and {1, 5, 6} (images 1, 5, 6); node 3 is unmatched."""
    return _graph([0, 2, 2, 0, 0, 2, 1, 0], [(0, 2), (4, 2), (5, 1), (6, 5)])


STAIR_K = 140  # candidates of two entries each: the boundary of candidates 127 | 128 is entry 255 | 256 of the sorted buffer


def _stairs():
    """Candidate k = {lo[k] in image k, hi[k] in image k + 1}, k = 0 .. STAIR_K - 1: in the sorted buffer the last entry of
    candidate k and the first of candidate k + 1 are the two keypoints of image k + 1 -- neighbours in ONE image that belong to
    two components.  (Which of the two comes first inside the image alternates.)  After them the one true conflict: x in image
    STAIR_K, y and z both in image STAIR_K + 1."""
    K = STAIR_K
    counts = [1] + [2] * K + [2]
    kp_ptr = np.concatenate([[0], np.cumsum(counts)])
    lo = np.array([0] + [kp_ptr[k] + (k % 2) for k in range(1, K)])
    hi = np.array([kp_ptr[k + 1] + (1 - (k + 1) % 2 if k + 1 < K else 0) for k in range(K)])
    x, y, z = kp_ptr[K] + 1, kp_ptr[K + 1], kp_ptr[K + 1] + 1
    return _graph(counts, [(h, l) for l, h in zip(lo, hi)] + [(x, y), (z, x)])


LIMIT_GRAPHS = {"big": lambda: _big(False), "big_long": lambda: _big(True), "sort_waves": _sort_waves, "ends": _ends, "stairs": _stairs}
LIMIT_NODE_TRACK = {"ends": [0, 1, 0, -1, 0, 1, 1]}
LIMIT_CAM_IDX = {"ends": [1, 2, 5, 1, 5, 6]}


@functools.lru_cache(maxsize=None)
def limit_graph(name):
    return LIMIT_GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def limit_reference(name):
    kp_ptr, kp_xy, edges, ok, min_length = limit_graph(name)
    return TR.build_tracks(kp_ptr, kp_xy, edges, ok, min_length)


# ---- an observation list as a matcher would deliver it ------------------------------------------------------------------
def matcher_output(pt_ptr, cam_idx, xy, n_images, seed, extra=5, edges="all", wrong=0.0):
    """Keypoints and matches of the list (pt_ptr, cam_idx, xy): every observation is a keypoint of its image, the keypoints of an
    image in a shuffled order with ``extra`` unmatched ones (random coordinates in the image's range) among them; a point's
    observations are matched in a chain (``edges="chain"``: consecutive cameras) or all with all ("all"); and ``wrong`` x the number
    of those matches are added between random keypoints of two different images that are not observations of one point.  All
    from the generator of ``seed``.  Returns a namespace: ``keypoints`` (a list of (n_i, 2)), ``matches`` (a dict {(k, l): (n, 2)},
    k < l ascending), ``wrong`` (the same keys: which matches are the added ones), ``kp_of_obs`` (n_obs,) (the keypoint of each
    observation, local to its image), ``n_true``, ``n_wrong``."""
    rng = np.random.default_rng(seed)
    pt_ptr, cam_idx, xy = np.asarray(pt_ptr), np.asarray(cam_idx), np.asarray(xy, np.float64).reshape(-1, 2)
    n_obs, n = len(cam_idx), len(pt_ptr) - 1
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    keypoints, kp_of_obs, point_of_kp = [], np.zeros(n_obs, np.int64), []
    for i in range(n_images):
        obs = np.nonzero(cam_idx == i)[0]
        perm = rng.permutation(len(obs) + extra)  # keypoint j is entry perm[j] of (the image's observations, then the extra ones)
        both = np.concatenate([xy[obs], lo + rng.random((extra, 2)) * (hi - lo)])
        keypoints.append(both[perm])
        inv = np.argsort(perm)
        kp_of_obs[obs] = inv[:len(obs)]
        point_of_kp.append(np.concatenate([pt[obs], np.full(extra, -1)])[perm])
    rows = []  # (k, l, kp in k, kp in l, wrong)
    for a in range(n):
        o = np.arange(pt_ptr[a], pt_ptr[a + 1])
        pairs = [(o[i], o[i + 1]) for i in range(len(o) - 1)] if edges == "chain" else [(o[i], o[j]) for i in range(len(o)) for j in range(i + 1, len(o))]
        rows += [(cam_idx[p], cam_idx[q], kp_of_obs[p], kp_of_obs[q], 0) for p, q in pairs]
    n_true = len(rows)
    n_wrong = int(round(wrong * n_true))
    while len(rows) < n_true + n_wrong:
        k, l = np.sort(rng.choice(n_images, 2, replace=False))
        a, b = rng.integers(len(keypoints[k])), rng.integers(len(keypoints[l]))
        if point_of_kp[k][a] < 0 or point_of_kp[k][a] != point_of_kp[l][b]:
            rows.append((k, l, a, b, 1))
    rows = np.array(rows, np.int64).reshape(-1, 5)
    rows = rows[np.lexsort((np.arange(len(rows)), rows[:, 1], rows[:, 0]))]
    keys, start = np.unique(rows[:, :2], axis=0, return_index=True)
    parts = np.split(rows, start[1:])
    return SimpleNamespace(keypoints=keypoints, matches={(int(k), int(l)): p[:, 2:4].copy() for (k, l), p in zip(keys, parts)},
                           wrong={(int(k), int(l)): p[:, 4] != 0 for (k, l), p in zip(keys, parts)}, kp_of_obs=kp_of_obs, n_true=n_true,
                           n_wrong=n_wrong)


@functools.lru_cache(maxsize=None)
def scene():
    from lib.synthetic import make_scene

    return make_scene(300, 8, vis_p=0.5)


@functools.lru_cache(maxsize=None)
def scene_matches(wrong):
    """matcher_output of the scene with all-pairs matches and the share ``wrong`` of wrong ones."""
    sc = scene()
    return matcher_output(sc.pt_ptr, sc.cam_idx, sc.xy, 8, seed=24, wrong=wrong)


INVARIANCE_WRONG = 0.03


@functools.lru_cache(maxsize=None)
def invariance_inputs():
    """Three statements of ONE edge set, as (image_pairs, kp_pairs): the matches of scene_matches(3 % wrong) as they come; permuted
    with half of them turned round; and with a third of them listed twice more, once turned round, in another order."""
    from lib.initialization import match_graph

    mo = scene_matches(INVARIANCE_WRONG)
    _, _, _, ip, kp = match_graph(mo.keypoints, mo.matches)
    rng = np.random.default_rng(3)
    perm, flip = rng.permutation(len(ip)), rng.random(len(ip)) < 0.5
    ip2, kp2 = ip[perm].copy(), kp[perm].copy()
    ip2[flip], kp2[flip] = ip2[flip][:, ::-1], kp2[flip][:, ::-1]
    dup = rng.random(len(ip)) < 1 / 3
    ip3 = np.concatenate([ip, ip[dup], ip[dup][:, ::-1]])
    kp3 = np.concatenate([kp, kp[dup], kp[dup][:, ::-1]])
    order = rng.permutation(len(ip3))
    return mo.keypoints, [(ip, kp), (ip2, kp2), (ip3[order], kp3[order])]


# ---- end to end: wrong matches, verified pair by pair, then tracks, bootstrap and Huber BA ---------------------------------
E2E_WRONG = 0.1        # of the true matches' number, added as wrong ones (the CPU reference lets a tenth of them through)
E2E_THRESHOLD = 0.01   # verify_matches and the three thresholds of bootstrap: ten times the scene's noise (tests/_ransac_cases.py)
E2E_HYP = 512
E2E_SEED = 1
E2E_DELTA = 5e-3       # the Huber scale of the BA that follows: five times the noise (tests/_tri_ransac_cases.py)
# The neighbouring end-to-end tests register all 8 cameras and end below the ground truth's cost with 20 % of EVERY camera's
# observations replaced (tests/_tri_ransac_cases.py: FRACTION).  The premise here is held to a quarter of that: of the
# observations of the tracks built from the verified matches, at most 5 % do not belong to the point most of their track
# belongs to; and the tracks must still be most of the scene's 300 points.
E2E_MAX_FOREIGN = 0.05
E2E_MIN_TRACKS = 240


def track_points(mo, cam_idx, kp_idx, pt_ptr):
    """(point (T,), foreign (n_obs,) bool): the scene point most of a track's observations (cam_idx, kp_idx) belong to (-1: none
    of them is an observation of the scene), and the observations that do not belong to it (an extra keypoint belongs to none)."""
    sc = scene()
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    point_of = {(int(c), int(k)): int(p) for c, k, p in zip(sc.cam_idx, mo.kp_of_obs, pt)}
    ids = np.array([point_of.get((int(c), int(k)), -1) for c, k in zip(cam_idx, kp_idx)], np.int64)
    top = np.full(len(pt_ptr) - 1, -1, np.int64)
    for a in range(len(pt_ptr) - 1):
        real = ids[pt_ptr[a]:pt_ptr[a + 1]]
        real = real[real >= 0]
        if len(real):
            values, counts = np.unique(real, return_counts=True)
            top[a] = values[np.argmax(counts)]
    return top, ids != np.repeat(top, np.diff(pt_ptr))


def foreign_share(mo, cam_idx, kp_idx, pt_ptr):
    """The share of the tracks' observations that do not belong to their track's point (track_points)."""
    return float(track_points(mo, cam_idx, kp_idx, pt_ptr)[1].sum()) / max(int(pt_ptr[-1]), 1)
