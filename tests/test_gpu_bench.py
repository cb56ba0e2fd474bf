"""bench.py's plain run on the GPU: the headline line and nothing measured beside it, and --dump-outputs writes
what the last timed step left committed -- parameters whose cost, recomputed by the oracle, is the dumped cost."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from lib.synthetic import make_scene
from oracle import ba_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_line_and_dumps_the_last_step(tmp_path):
    n = 20_000
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--points", str(n), "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "it/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(1e3 / d["ms_per_step"])
    # nothing but the timed steps was measured: no per-kernel pass of its own, no public-API run, no CPU leg
    assert d["optimize_api"] is None and "cpu_baseline" not in d and set(d["kernel_ms_per_step"]) == {"resid_jac", "schur"}

    a = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(a) == ["cameras_R", "cameras_f", "cameras_t", "cameras_u", "cost", "points_X"]
    assert all(v.dtype == np.float64 for v in a.values())
    sc = make_scene(n, 100, vis_p=0.1, point_range=(0, n))
    assert a["points_X"].shape == (n, 3) and a["cameras_R"].shape == (100, 3, 3) and a["cost"].shape == (1,)
    E = float(a["cost"][0])
    assert np.sqrt(E / sc.n_obs) == pytest.approx(d["rmse_end"], rel=1e-12)
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    E_oracle = O.cost(a["points_X"], a["cameras_f"], a["cameras_u"], a["cameras_t"], a["cameras_R"], 1.0, pt, sc.cam_idx, sc.xy)
    assert E_oracle == pytest.approx(E, rel=1e-9)
