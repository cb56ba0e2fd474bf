"""Device time of one LM step with a robust loss against the squared loss, per phase (mvba_set_profiling: K1, K3a, K3,
solve, back-substitution + trial cost), at config 3 (1 M points x 100 cameras x 10 %).  A robust engine never takes the
slot form of K3, so the squared loss is timed in the unit form too (MVBA_SCHUR=pairs), and in its default form for reference.

    python tools/time_robust.py [--steps 10] [--reps 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-reconstruction-from-multi-view-exp_amd"), ROOT]

from lib._mvba import HipEngine  # noqa: E402
from lib.bundle_adjustment import to_gauge_frame  # noqa: E402
from lib.synthetic import make_scene  # noqa: E402

PHASES = ("resid_jac", "point_inv", "schur", "solve", "backsub_cost")


def one(sc, X, R, t, loss, scale, schur, steps):
    if schur:
        os.environ["MVBA_SCHUR"] = schur
    eng = HipEngine(sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis, loss=loss, loss_scale=scale)
    os.environ.pop("MVBA_SCHUR", None)
    eng.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    eng.linearize()
    eng.try_step(1e-4)  # warm-up
    eng.set_profiling(True)
    eng.reset_stats()
    for _ in range(steps):  # the same step again and again: linearise at the committed state, one trial
        eng.linearize()
        eng.try_step(1e-4)
    st = eng.stats()
    form = eng.schur_info()["kernel"]
    eng.close()
    ms = {k: st[k]["ms"] / steps for k in PHASES}
    return {"loss": loss, "form": form, "per_step_ms": {k: round(v, 4) for k, v in ms.items()}, "step_ms": round(sum(ms.values()), 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    sc = make_scene(1_000_000, 100, vis_p=0.1)
    X, R, t = to_gauge_frame(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    # (make_scene's image noise is 1e-3 and its initial state ~1e-2 off: delta = 5e-3 puts most rows on the robust branch)
    runs = [("squared", None, None), ("squared", None, "pairs"), ("huber", 5e-3, None), ("cauchy", 5e-3, None)]
    for rep in range(a.reps):
        for loss, scale, schur in runs:
            r = one(sc, X, R, t, loss, scale, schur, a.steps)
            r["rep"] = rep
            print(json.dumps(r), flush=True)
