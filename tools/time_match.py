"""mvba_match_descriptors at config 3's scale: 100 images x 10^5 keypoints x 128 random bytes, all of it uploaded
by every call.  Two loads: the 16 most co-visible image pairs of a config-3-like scene in ONE call, and the first of them alone;
ratio 0.8 with the mutual check, so a pair is 2 x 10^10 distances.  Per call the entry point's own four laps (checks and upload;
distances; tests and compaction; download and the rest) and the wall time; median of --reps; the distances per second of the
`distances` lap.  Beside it the NumPy restatement of the same definition on the host's CPUs -- the dot products as a float32
GEMM in blocks (exact: every partial sum is an integer below 2^24 at dim <= 256), the nearest two by argpartition -- on the first
--host-queries queries of the first pair, forwards only, compared with the device's per-query arrays and scaled by its rate.
--keypoints scales the load: the first device run of a new build is `--keypoints 2000 --reps 1`, alone, under a time limit of
its own.

    python tools/time_match.py [--images 100] [--keypoints 100000] [--dim 128] [--pairs 16] [--reps 5] [--host-queries 8192]
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

LAPS = ("upload", "distances", "tests", "download")


def covisible_pairs(m, count):
    """The ``count`` image pairs k < l that share the most points of a config-3-like scene (a tenth of its points: the order of
    the pairs is what matters here)."""
    sc = make_scene(100_000, m, vis_p=0.1)
    seen = np.zeros((m, sc.n_points), np.float32)
    seen[sc.cam_idx, np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))] = 1
    shared = np.triu(seen @ seen.T, 1)
    top = np.argsort(-shared, axis=None, kind="stable")[:count]
    return np.stack(np.unravel_index(top, shared.shape), axis=1).astype(np.int32)


def host_nearest_two(A, B, block=2048):
    """(best, best2, second2) of queries A against candidates B, as tests/_match_ref.py defines them, in blocks of queries."""
    Bf, bn = B.astype(np.float32), (B.astype(np.int64) ** 2).sum(axis=1)
    best, best2, second2 = (np.empty(len(A), np.int32) for _ in range(3))
    for at in range(0, len(A), block):
        a = A[at:at + block]
        D = bn[None, :] - 2 * (a.astype(np.float32) @ Bf.T).astype(np.int64)  # without |a|^2: it moves no argmin
        two = np.argpartition(D, 1, axis=1)[:, :2]
        rows = np.arange(len(a))
        d = D[rows[:, None], two]
        low = d.min(axis=1)
        ties = (D == low[:, None])  # a tie goes to the smaller index, and makes the second equal to the best
        first = ties.argmax(axis=1)
        an = (a.astype(np.int64) ** 2).sum(axis=1)
        best[at:at + block], best2[at:at + block] = first, low + an
        second2[at:at + block] = np.where(ties.sum(axis=1) > 1, low, d.max(axis=1)) + an
    return best, best2, second2


def timed(kp_ptr, desc, pairs, reps, **kw):
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = _mvba.match_descriptors(kp_ptr, desc, pairs, **kw)
        runs.append({"wall_ms": 1e3 * (time.perf_counter() - t0), **out["timings_ms"]})
    med = {k: round(statistics.median(r[k] for r in runs), 3) for k in ("wall_ms",) + LAPS}
    return out, med, (round(min(r["distances"] for r in runs), 3), round(max(r["distances"] for r in runs), 3))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--keypoints", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-queries", type=int, default=8192)
    a = ap.parse_args()
    m, n = a.images, a.keypoints
    rng = np.random.default_rng(25)
    desc = rng.integers(0, 256, (m * n, a.dim), dtype=np.uint8)
    kp_ptr = np.arange(m + 1, dtype=np.int64) * n
    pairs = covisible_pairs(m, a.pairs)
    _mvba.match_descriptors(np.array([0, 64, 128]), desc[:128], [[0, 1]])  # warm-up: the first call loads the code objects
    for name, pl in (("pairs together", pairs), ("one pair", pairs[:1])):
        out, med, spread = timed(kp_ptr, desc, pl, a.reps, ratio=0.8, mutual=True, want_nn=(name == "one pair"))
        n_dist = 2 * len(pl) * n * n
        print(json.dumps({"load": name, "n_pairs": len(pl), "images": m, "keypoints": n, "dim": a.dim, "descriptor_bytes": int(desc.nbytes),
                          "distances": n_dist, "median_ms": med, "distances_ms_min_max": spread,
                          "distances_per_s": round(n_dist / (1e-3 * med["distances"]), 0), "distances_per_s_wall": round(n_dist / (1e-3 * med["wall_ms"]), 0),
                          **{k: out[k] for k in _mvba.MATCH_COUNTS}, "reps": a.reps}), flush=True)
    k, l = pairs[0]
    hq = min(a.host_queries, n)
    A, B = desc[kp_ptr[k]:kp_ptr[k] + hq], desc[kp_ptr[l]:kp_ptr[l + 1]]
    host = []
    for _ in range(min(a.reps, 3)):
        t0 = time.perf_counter()
        best, best2, second2 = host_nearest_two(A, B)
        host.append(time.perf_counter() - t0)
    t = statistics.median(host)
    same = bool(np.array_equal(best, out["nn_best"][:hq]) and np.array_equal(best2, out["nn_dist2"][:hq]) and np.array_equal(second2, out["nn_second2"][:hq]))
    print(json.dumps({"host_baseline": "NumPy: float32 GEMM in blocks of 2048 queries, argpartition", "queries": hq, "candidates": len(B),
                      "median_s": round(t, 3), "distances_per_s": round(hq * len(B) / t, 0), "one_pair_both_ways_s": round(2 * n * n / (hq * len(B) / t), 1),
                      "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "same_answers": same, "reps": min(a.reps, 3)}), flush=True)
