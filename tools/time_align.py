"""mvba_align_robust on config 3's points: src = the 1 M ground-truth points, dst = a similarity of them (s = 2.5)
plus Gaussian noise 1e-3 s, 30 % of the rows replaced by uniform positions in dst's box, threshold 0.01 s, H = 512, two refits.  Per
call the device time between two events on the stream the kernels run in and the call's own four laps (upload and compaction;
hypotheses and scoring; refits; rest); median of --reps.  Beside it mvba_align on the clean rows, and the same least squares on the
host by np.linalg.svd of the 3 x 3 cross-covariance (Umeyama).  --points scales the point count: the first device run of a new
build is `--points 0.001 --reps 1`, alone, under a time limit of its own.

    python tools/time_align.py [--reps 5] [--points 1.0] [--hyp 512]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-reconstruction-from-multi-view-exp_amd"), ROOT]

from lib import _mvba  # noqa: E402
from lib.synthetic import make_scene  # noqa: E402

LAPS = ("upload", "score", "refit", "other")
SCALE, TAU = 2.5, np.array([10.0, -3.0, 4.0])


def correspondences(src, frac, seed=7):
    """(dst, bad): the similarity of src plus noise, a seeded fraction of the rows replaced by uniform positions in dst's box."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    Q = Q if np.linalg.det(Q) > 0 else -Q
    dst = SCALE * src @ Q.T + TAU + rng.normal(0.0, 1e-3 * SCALE, src.shape)
    bad = rng.random(len(src)) < frac
    lo, hi = dst.min(axis=0), dst.max(axis=0)
    dst[bad] = lo + (hi - lo) * rng.random((int(bad.sum()), 3))
    return dst, bad


def host_fit(x, y):
    """Umeyama's least squares on the host: (s, Q, tau)."""
    mx, my = x.mean(axis=0), y.mean(axis=0)
    xc, yc = x - mx, y - my
    U, sv, Vt = np.linalg.svd(yc.T @ xc)
    d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0
    Q = U @ np.diag([1.0, 1.0, d]) @ Vt
    s = (sv[0] + sv[1] + d * sv[2]) / (xc * xc).sum()
    return s, Q, my - s * Q @ mx


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
    n = int(1_000_000 * a.points)
    src = np.ascontiguousarray(make_scene(n, 100, vis_p=0.1).X_gt)
    dst, bad = correspondences(src, 0.3)
    thr = 0.01 * SCALE
    _mvba.align_robust(src[:1000], dst[:1000], thr, n_hypotheses=a.hyp, seed=1)  # warm-up: the first call loads the code objects
    _mvba.align(src[:1000], dst[:1000])
    xc, yc = np.ascontiguousarray(src[~bad]), np.ascontiguousarray(dst[~bad])
    robust, plain, host = [], [], []
    for _ in range(a.reps):
        out, ms = timed(_mvba.align_robust, src, dst, thr, n_hypotheses=a.hyp, seed=1, n_refit=2)
        robust.append({"device_ms": ms, **out["timings_ms"]})
        fit, ms = timed(_mvba.align, xc, yc)
        plain.append(ms)
        t0 = time.perf_counter()
        s, Q, tau = host_fit(xc, yc)
        host.append(1e3 * (time.perf_counter() - t0))
    med = {k: round(statistics.median(x[k] for x in robust), 3) for k in ("device_ms",) + LAPS}
    exact = bool(np.array_equal(out["inlier"], ~bad))
    print(json.dumps({"scene": "config3 points", "points": n, "n_hypotheses": a.hyp, "n_refit": 2, "call": "align_robust", "median_ms": med,
                      "device_ms_min_max": (round(min(x["device_ms"] for x in robust), 3), round(max(x["device_ms"] for x in robust), 3)),
                      "status": out["status"], "n_inliers": out["n_inliers"], "n_clean": int((~bad).sum()), "inliers_are_the_clean_rows": exact,
                      "best": out["best"], "rms": float(out["quality"][0]), "reps": a.reps}), flush=True)
    print(json.dumps({"call": "align (clean rows)", "points": len(xc), "median_ms": round(statistics.median(plain), 3),
                      "host_numpy_svd_median_ms": round(statistics.median(host), 3),
                      "device_vs_host": float(max(abs(fit["s"] - s), np.abs(fit["Q"] - Q).max(), np.abs(fit["tau"] - tau).max())),
                      "robust_vs_host": float(max(abs(out["s"] - s), np.abs(out["Q"] - Q).max(), np.abs(out["tau"] - tau).max())), "reps": a.reps}), flush=True)
