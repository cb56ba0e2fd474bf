"""mvba_build_tracks on config 3's observation list turned into keypoints and matches: 1 M points x 100 cameras x
10 % = 10 M keypoints, every image's keypoints in a shuffled order; a point's observations matched in a chain (--edges chain: 9 M
edges) or all with all (--edges all: about 45 M), plus 1 % as many wrong edges between random keypoints, the list shuffled and half
of it turned round.  Per call the entry point's own four laps (upload with the checks; labels; layout; download and the rest) and
the wall time; median of --reps; the label rounds; what was dropped, with the size of the largest dropped component.  Beside it the
same answer on the host -- scipy.sparse.csgraph.connected_components, then NumPy grouping (bincount, lexsort) -- where scipy is
there, compared with the device's arrays.  --points scales the point count: the first device run of a new build is
`--points 0.001 --reps 1`, alone, under a time limit of its own.

    python tools/time_tracks.py [--edges chain|all] [--reps 3] [--points 1.0] [--wrong 0.01]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-reconstruction-from-multi-view-exp_amd"), ROOT]

from lib import _mvba  # noqa: E402
from lib.synthetic import make_scene  # noqa: E402

LAPS = ("upload", "labels", "layout", "download")


def match_graph_of(pt_ptr, cam_idx, xy, m, how, wrong, seed=5):
    """(kp_ptr, kp_xy, edges) of the list: nodes image-major with a shuffled order inside an image, the matches of every point, the
    wrong ones, all of it in a random order and orientation."""
    rng = np.random.default_rng(seed)
    n_obs = len(cam_idx)
    order = np.lexsort((rng.random(n_obs), cam_idx))  # node v is observation order[v]
    node = np.empty(n_obs, np.int32)
    node[order] = np.arange(n_obs, dtype=np.int32)
    kp_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam_idx, minlength=m))]).astype(np.int64)
    kp_xy = np.ascontiguousarray(xy[order])
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    parts = []
    for step in range(1, int(np.diff(pt_ptr).max()) if how == "all" else 2):  # observations `step` apart inside one point
        same = pt[step:] == pt[:-step]
        parts.append(np.stack([node[:-step][same], node[step:][same]], axis=1))
    true = np.concatenate(parts)
    bad = rng.integers(0, n_obs, (int(round(wrong * len(true))), 2)).astype(np.int32)
    edges = np.concatenate([true, bad])
    edges = edges[rng.permutation(len(edges))]
    flip = rng.random(len(edges)) < 0.5
    edges[flip] = edges[flip][:, ::-1]
    return kp_ptr, kp_xy, np.ascontiguousarray(edges), len(true), len(bad)


def min_labels(n, edges):
    """The smallest node of every node's component, NumPy only (for the small graph of the dropped components)."""
    label = np.arange(n)
    while True:
        low = np.minimum(label[edges[:, 0]], label[edges[:, 1]])
        new = label.copy()
        np.minimum.at(new, edges[:, 0], low)
        np.minimum.at(new, edges[:, 1], low)
        while not (new[new] == new).all():
            new = new[new]
        if (new == label).all():
            return label
        label = new


def largest_dropped(node_track, edges):
    """The node count of the largest component among those of node_track == -3."""
    dropped = np.nonzero(node_track == -3)[0]
    if len(dropped) == 0:
        return 0
    local = np.full(len(node_track), -1, np.int64)
    local[dropped] = np.arange(len(dropped))
    e = local[edges[node_track[edges[:, 0]] == -3]]  # (both ends of an edge lie in one component)
    return int(np.bincount(min_labels(len(dropped), e)).max())


def host_tracks(kp_ptr, edges, min_length=2):
    """(pt_ptr, obs_node) on the host: scipy's connected components, then grouping by bincount and lexsort."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    m, n = len(kp_ptr) - 1, int(kp_ptr[-1])
    _, comp = connected_components(coo_matrix((np.ones(len(edges), np.int8), (edges[:, 0], edges[:, 1])), shape=(n, n)), directed=False)
    size = np.bincount(comp)
    cand = (size >= max(min_length, 2)) & (size <= m)
    nodes = np.nonzero(cand[comp])[0]
    nodes = nodes[np.argsort(comp[nodes], kind="stable")]  # ascending node inside a component
    image = np.searchsorted(kp_ptr, nodes, side="right") - 1
    same = (comp[nodes][1:] == comp[nodes][:-1]) & (image[1:] == image[:-1])
    bad = np.zeros(len(size), bool)
    bad[comp[nodes][1:][same]] = True
    nodes = nodes[~bad[comp[nodes]]]
    first = np.full(len(size), n, np.int64)  # tracks in ascending order of their smallest node
    np.minimum.at(first, comp[nodes], nodes)
    nodes = nodes[np.argsort(first[comp[nodes]], kind="stable")]
    starts = np.nonzero(np.concatenate([[True], comp[nodes][1:] != comp[nodes][:-1]]))[0]
    return np.concatenate([starts, [len(nodes)]]).astype(np.int64), nodes.astype(np.int32)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", choices=("chain", "all"), default="chain")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=float, default=1.0)
    ap.add_argument("--wrong", type=float, default=0.01)
    a = ap.parse_args()
    n, m = int(1_000_000 * a.points), 100
    sc = make_scene(n, m, vis_p=0.1)
    kp_ptr, kp_xy, edges, n_true, n_bad = match_graph_of(sc.pt_ptr, sc.cam_idx, sc.xy, m, a.edges, a.wrong)
    _mvba.build_tracks(kp_ptr[:3], kp_xy[:kp_ptr[2]], np.zeros((0, 2), np.int32))  # warm-up: the first call loads the code objects
    runs = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = _mvba.build_tracks(kp_ptr, kp_xy, edges)
        runs.append({"wall_ms": 1e3 * (time.perf_counter() - t0), **out["timings_ms"]})
    res = {"scene": "config3 list", "edges": a.edges, "n_nodes": int(kp_ptr[-1]), "n_edges": len(edges), "n_true": n_true, "n_wrong": n_bad,
           "median_ms": {k: round(statistics.median(r[k] for r in runs), 3) for k in ("wall_ms",) + LAPS},
           "wall_ms_min_max": (round(min(r["wall_ms"] for r in runs), 3), round(max(r["wall_ms"] for r in runs), 3)),
           **{k: out[k] for k in _mvba.TRACK_COUNTS}, "largest_dropped_component": largest_dropped(out["node_track"], edges), "reps": a.reps}
    print(json.dumps(res), flush=True)
    try:
        import scipy  # noqa: F401
    except ImportError:
        print(json.dumps({"host_baseline": "skipped: no scipy"}), flush=True)
    else:
        host = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            pt_ptr, obs_node = host_tracks(kp_ptr, edges)
            host.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps({"host_baseline": "scipy connected_components + NumPy grouping", "median_ms": round(statistics.median(host), 3),
                          "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "same_tracks": bool(np.array_equal(pt_ptr, out["pt_ptr"]) and
                                                                                  np.array_equal(obs_node, out["obs_node"])),
                          "reps": a.reps}), flush=True)
