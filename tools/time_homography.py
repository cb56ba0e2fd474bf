"""mvba_homography_robust against mvba_two_view_robust on one list: config 3's observations (1 M points x 100
cameras x 10 %), the 16 most co-visible pairs, 30 % of image l of every pair replaced by uniform positions, H = 512, two
refits.  The two calls alternate, so that a drift of the machine hits both; per call the device time between two events on the
stream the kernels run in, and the call's own four laps (upload; compaction, normalisation, hypotheses and scoring; refits;
rest); median of --reps.  The hypothesis and the scoring kernels by themselves are a kernel trace of this very program
(one run under the profiler with --reps 2, read with tools/kstats.py).  --points scales the point count.

    python tools/time_homography.py [--reps 5] [--points 1.0] [--hyp 512]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-reconstruction-from-multi-view-exp_amd"), ROOT]

from lib import _mvba  # noqa: E402
from lib.initialization import covisibility  # noqa: E402
from lib.synthetic import make_scene  # noqa: E402

LAPS = ("upload", "score", "refit", "other")


def replace_in_l(sc, pairs, frac, seed=7):
    """xy with a seeded fraction of every pair's image-l observations replaced by uniform positions inside the bounds of xy."""
    xy = np.array(sc.xy, np.float64).reshape(-1, 2)
    rng = np.random.default_rng(seed)
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    for l in sorted({int(p[1]) for p in pairs}):
        obs = np.nonzero(sc.cam_idx == l)[0]
        hit = obs[rng.random(len(obs)) < frac]
        xy[hit] = lo + rng.random((len(hit), 2)) * (hi - lo)
    return xy


def timed(fn, *args, **kw):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    out = fn(*args, **kw)
    ev[1].record()
    torch.cuda.synchronize()
    return out, ev[0].elapsed_time(ev[1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=float, default=1.0)
    ap.add_argument("--hyp", type=int, default=512)
    a = ap.parse_args()
    n, m = int(1_000_000 * a.points), 100
    sc = make_scene(n, m, vis_p=0.1)
    count = covisibility(sc.pt_ptr, sc.cam_idx, m)
    ks, ls = np.triu_indices(m, 1)
    order = np.argsort(-count[ks, ls], kind="stable")[:16]
    pairs = np.stack([ks[order], ls[order]], axis=1).astype(np.int32)
    xy = replace_in_l(sc, pairs, 0.3)
    calls = (("two_view_robust", _mvba.two_view_robust), ("homography_robust", _mvba.homography_robust))
    runs = {name: [] for name, _ in calls}
    for name, fn in calls:  # warm-up: the first call loads the code objects
        fn(sc.pt_ptr, sc.cam_idx, xy, m, pairs[:1], 0.01, n_hypotheses=a.hyp, seed=1, return_inliers=False)
    for _ in range(a.reps):
        for name, fn in calls:
            out, ms = timed(fn, sc.pt_ptr, sc.cam_idx, xy, m, pairs, 0.01, n_hypotheses=a.hyp, seed=1, n_refit=2, return_inliers=False)
            runs[name].append({"device_ms": ms, **out["timings_ms"], "n_inliers": out["n_inliers"].tolist(), "status": out["status"].tolist()})
    for name, _ in calls:
        r = runs[name]
        med = {k: round(statistics.median(x[k] for x in r), 3) for k in ("device_ms",) + LAPS}
        print(json.dumps({"scene": "config3", "points": n, "cameras": m, "pairs": len(pairs), "n_shared": [int(count[k, l]) for k, l in pairs][:4],
                          "n_hypotheses": a.hyp, "call": name, "median_ms": med,
                          "device_ms_min_max": (round(min(x["device_ms"] for x in r), 3), round(max(x["device_ms"] for x in r), 3)),
                          "status": r[0]["status"], "n_inliers": r[0]["n_inliers"][:4], "reps": a.reps}), flush=True)
