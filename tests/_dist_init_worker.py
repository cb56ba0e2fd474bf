"""Worker for tests/test_gpu_init.py: HipEngine.triangulate in a world-size-2 job on ONE GPU over the host-staged
transport (the pattern of _dist_gpu_worker.py).  Each rank triangulates its own points and talks to nobody; the result
must be the stateless call's on the whole list."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-reconstruction-from-multi-view-exp_amd"), ROOT):
    sys.path.insert(0, p)

import torch.distributed as dist  # noqa: E402

from lib import _distributed as D  # noqa: E402
from lib import _mvba  # noqa: E402
from lib.bundle_adjustment import intrinsics_from  # noqa: E402
from lib.synthetic import make_scene  # noqa: E402
from oracle import ba_oracle as O  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    m = 6
    sc = make_scene(700, m, vis_p=0.5, project="numpy")
    lo, hi = D.partition_points(sc.pt_ptr, world)[rank]
    pt_ptr, cam, xy = D.slice_observations(sc.pt_ptr, sc.cam_idx, sc.xy, lo, hi)
    _, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    f, u = sc.init_K[:, 0, 0], sc.init_K[:, :2, 2]
    eng = _mvba.HipEngine(hi - lo, m, pt_ptr, cam, xy, 1.0, sc.axis)
    D.attach_host_comm(eng)
    eng.set_params(np.zeros((hi - lo, 3)), f, u, t, R)
    q, st, _ = eng.triangulate(2)
    X = eng.get_params()[0]
    X1, q1, st1, _ = _mvba.triangulate(intrinsics_from(f, u, 1.0), R, t, sc.pt_ptr, sc.cam_idx, sc.xy, n_refine=2)
    assert (st == 0).all() and (st1 == 0).all()
    assert np.array_equal(X, X1[lo:hi]) and np.array_equal(q, q1[lo:hi])  # the same kernel on the same numbers
    E = eng.cost()  # (a collective: both ranks get here, the sharded engine works on from the triangulated points)
    assert np.isfinite(E) and E < 1e-2 * sc.n_obs
    dist.barrier()
    if rank == 0:
        print("DIST_INIT_OK", E)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
