"""Device time of one LM step with held points against the engine without a mask, per phase
(mvba_set_profiling: K1, K3a, K3, solve, back-substitution + trial cost), and mvba_covariance's point pass: no mask, every
second point held, all points held.  Only K3a and the point pass change with the mask; the Schur kernel does the same work
on rows of zeros.  Scene: config 3 (1 M points x 100 cameras x 10 %); --points scales the point count.

    python tools/time_point_hold.py [--steps 10] [--reps 5] [--points 1.0] [--no-covariance]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-reconstruction-from-multi-view-exp_amd"), ROOT]

from lib._mvba import HipEngine  # noqa: E402
from lib.bundle_adjustment import to_gauge_frame  # noqa: E402
from lib.synthetic import make_scene  # noqa: E402

PHASES = ("resid_jac", "point_inv", "schur", "solve", "backsub_cost")


def one(eng, steps):
    eng.linearize()
    eng.try_step(1e-4)  # warm-up
    eng.set_profiling(True)
    eng.reset_stats()
    for _ in range(steps):  # the same step again and again: linearise at the committed state, one trial
        eng.linearize()
        eng.try_step(1e-4)
    st = eng.stats()
    eng.set_profiling(False)
    return {k: st[k]["ms"] / steps for k in PHASES}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=float, default=1.0)
    ap.add_argument("--no-covariance", action="store_true")
    a = ap.parse_args()
    n, m, p = int(1_000_000 * a.points), 100, 0.1
    sc = make_scene(n, m, vis_p=p)
    X, R, t = to_gauge_frame(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    eng = HipEngine(n, m, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis)
    eng.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    cases = (("no_mask", None), ("half_held", np.arange(n) % 2 == 0), ("all_held", np.ones(n, bool)))
    runs = {label: [] for label, _ in cases}
    for _ in range(a.reps):  # the cases alternate, so that a drift of the machine hits all of them
        for label, mask in cases:
            eng.set_point_hold(mask)
            runs[label].append(one(eng, a.steps))
    for label, _ in cases:
        med = {k: round(statistics.median(r[k] for r in runs[label]), 4) for k in PHASES}
        lo_hi = {k: (round(min(r[k] for r in runs[label]), 4), round(max(r[k] for r in runs[label]), 4)) for k in ("point_inv", "schur")}
        print(json.dumps({"scene": "config3", "points": n, "cameras": m, "mask": label, "per_step_ms_median": med,
                          "step_ms": round(sum(med.values()), 4), "min_max_ms": lo_hi, "reps": a.reps, "steps": a.steps}), flush=True)
    if not a.no_covariance:
        cov = {label: [] for label, _ in cases[:2]}
        eng.set_point_hold(None)
        eng.covariance(points=True, cameras=False)  # warm-up: the first call allocates
        for _ in range(a.reps):
            for label, mask in cases[:2]:
                eng.set_point_hold(mask)
                cov[label].append(eng.covariance(points=True, cameras=False)["timings_ms"])
        for label, _ in cases[:2]:
            med = {k: round(statistics.median(r[k] for r in cov[label]), 4) for k in ("schur", "factor", "inverse", "points")}
            print(json.dumps({"scene": "config3", "mask": label, "covariance_ms_median": med,
                              "points_min_max_ms": (round(min(r["points"] for r in cov[label]), 4), round(max(r["points"] for r in cov[label]), 4)),
                              "reps": a.reps}), flush=True)
    eng.close()
