"""Device time of mvba_covariance per phase (timings_ms: linearise+Schur, factor, inverse, point pass) at config 3
(1 M points x 100 cameras x 10 %, D = 893) and at the config-4 shard shape (400 k points x 500 cameras x 5 %, D = 4493).

The point pass is priced by the bytes it gathers: per unordered observation pair of a point one camera block of the
covariance table (656 B) and two 128-byte records, against the gathered-row rate of MI355X_MICROARCH.md ('Indexed rows':
8.6 TB/s from a table that misses L2, 16.8-18.8 TB/s from one an XCD's L2 holds).

    python tools/time_covariance.py [--reps 5] [--only c3|c4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-reconstruction-from-multi-view-exp_amd"), ROOT]

from lib._mvba import HipEngine  # noqa: E402
from lib.bundle_adjustment import to_gauge_frame  # noqa: E402
from lib.synthetic import make_scene  # noqa: E402

SHAPES = {"c3": (1_000_000, 100, 0.1), "c4": (400_000, 500, 0.05)}


def run(name, reps):
    n, m, p = SHAPES[name]
    t0 = time.perf_counter()
    sc = make_scene(n, m, vis_p=p)
    X, R, t = to_gauge_frame(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    eng = HipEngine(sc.n_points, m, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis)
    eng.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    setup = time.perf_counter() - t0
    eng.covariance()  # first call: the lazy allocations
    rows = []
    for _ in range(reps):
        w0 = time.perf_counter()
        out = eng.covariance(points=True, cameras=True)
        rows.append(dict(out["timings_ms"], wall=1e3 * (time.perf_counter() - w0)))
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    deg = np.diff(sc.pt_ptr).astype(np.float64)
    pairs = float((deg * (deg + 1) / 2).sum())
    gathered = pairs * (656 + 2 * 128)
    res = {"shape": name, "n_points": sc.n_points, "m": m, "n_obs": int(sc.n_obs), "D": 9 * m - 7, "setup_s": round(setup, 1),
           "median_ms": {k: round(v, 3) for k, v in med.items()},
           "device_total_ms": round(sum(med[k] for k in ("schur", "factor", "inverse", "points")), 3),
           "point_pass": {"pairs": int(pairs), "gathered_GB": round(gathered / 1e9, 2),
                          "rate_TBps": round(gathered / (med["points"] * 1e-3) / 1e12, 2),
                          "ms_at_8.6TBps": round(gathered / 8.6e12 * 1e3, 2)}}
    print(json.dumps(res), flush=True)
    eng.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=sorted(SHAPES))
    a = ap.parse_args()
    for name in ([a.only] if a.only else ["c3", "c4"]):
        run(name, a.reps)
