"""Initial estimates for bundle adjustment when visibility is sparse: triangulate every point from the cameras that
are known, resect every camera from the points that are known -- the two steps that extend a reconstruction.  Both run
on the MI355X (``mvba_triangulate``, ``mvba_resect``: csrc/mvba_init.h); there is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _mvba


def triangulate_points(pt_ptr, cam_idx, xy, K, R, t, n_refine: int = 2):
    """X (N, 3) from the cameras K, R, t (the conventions of ``_mvba.project``: P_k = K_k [R_k^T | -R_k^T t_k]) and the
    CSR-by-point observation list; ``pt_ptr=None`` with xy (N, m, 2) is the dense grid.  ``xy`` is in the units ``K``
    projects to: for raw image coordinates and the (f, u) of ``BundleAdjuster`` pass ``K[:, 2, 2] = 1`` (the ``init_K`` of
    ``BundleAdjuster`` carries f0 there and projects to x / f0: ``engine_intrinsics`` below undoes that), whatever f0 is.
    The linear (DLT) solution, then
    ``n_refine`` Gauss-Newton steps on the reprojection error.  ``info``: ``status`` (N,) -- 0 ok, 1 fewer than two
    observations, 2 no parallax, 3 at infinity or not finite; X is NaN where it is not 0 -- ``quality`` (N, 3) -- RMS
    reprojection residual in units of xy, smallest depth over the point's cameras (<= 0: behind a camera), largest angle
    in radians between two of its viewing rays -- and ``timings_ms``.  ``info["status"] == 0`` is the filter for
    ``BundleAdjuster.from_observations(init_X=None)``."""
    X, quality, status, tm = _mvba.triangulate(K, R, t, pt_ptr, cam_idx, xy, n_refine=n_refine)
    return X, {"status": status, "quality": quality, "timings_ms": tm}


def engine_intrinsics(K):
    """``K`` (m, 3, 3) with its third row divided by ``K[2, 2]``: the matrix that projects to the raw image coordinates the
    adjuster is given, out of an ``init_K`` = [[f,0,u],[0,f,v],[0,0,f0]] (which projects to x / f0)."""
    K = np.array(K, dtype=np.float64)
    K[..., 2, :] = K[..., 2, :] / K[..., 2, 2:3]
    return K


def decompose_projection(P, f0: float = 1.0):
    """(K, R, t) of camera matrices P (m, 3, 4) or (3, 4) that project to RAW image coordinates (the xy ``BundleAdjuster``
    is given), in the form ``BundleAdjuster`` takes as ``init_K``, ``init_R``, ``init_t``: RQ of P[:, :3] with a positive
    diagonal, P[:, :3] = K' R^T with K'[2, 2] = 1; f = (K'00 + K'11) / 2, u = (K'02, K'12), the skew dropped; K =
    [[f,0,u],[0,f,v],[0,0,f0]] -- the engine's model, whose (f, u) do not depend on f0: it projects to x / f0, and f0 sits in
    K[2, 2] alone --; R with columns = the camera axes, t the camera centre.  With f0 = 1, P = K [R^T | -R^T t]."""
    P = np.asarray(P, dtype=np.float64)
    single = P.ndim == 2
    P = P.reshape(-1, 3, 4)
    m = P.shape[0]
    K, R, t = np.zeros((m, 3, 3)), np.empty((m, 3, 3)), np.empty((m, 3))
    flip = np.eye(3)[::-1]
    for k in range(m):
        M = P[k, :, :3]
        if np.linalg.det(M) < 0:  # (P is defined up to scale: the sign that makes R a rotation)
            M = -M
        q, r = np.linalg.qr((flip @ M).T)  # RQ by QR of the row-reversed transpose
        Ku, Rc = flip @ r.T @ flip, flip @ q.T
        s = np.sign(np.diag(Ku))
        s[s == 0] = 1.0
        Ku, Rc = Ku * s, s[:, None] * Rc  # M = Ku Rc, Ku upper triangular with a positive diagonal, Rc = R^T
        Ku = Ku / Ku[2, 2]
        f = 0.5 * (Ku[0, 0] + Ku[1, 1])
        K[k] = [[f, 0.0, Ku[0, 2]], [0.0, f, Ku[1, 2]], [0.0, 0.0, f0]]
        R[k] = Rc.T
        t[k] = -np.linalg.solve(P[k, :, :3], P[k, :, 3])
    return (K[0], R[0], t[0]) if single else (K, R, t)


def resect_cameras(X, pt_ptr, cam_idx, xy, n_images: int, f0: float = 1.0, point_ok=None):
    """(K, R, t, info) of every camera from the points X (N, 3) it sees: the normalised DLT on the device, then
    ``decompose_projection``: ``xy`` are the raw image coordinates the adjuster is given, and K comes back as its ``init_K``
    (f, u in those units, f0 in K[2, 2]).  ``pt_ptr=None`` with xy (N, m, 2) is the dense grid.  ``point_ok`` (N,) marks the points to use (default: those whose X is finite).  ``info``:
    ``status`` (m,) -- 0 ok, 1 fewer than 6 usable observations, 2 degenerate (e.g. coplanar points); K, R, t are NaN where
    it is not 0 --, ``quality`` (m, 2) -- RMS reprojection residual of the camera's used observations, eigenvalue ratio
    lambda_1 / lambda_2 (small: well determined) --, ``P`` (m, 3, 4) and ``timings_ms``."""
    P, quality, status, tm = _mvba.resect(X, pt_ptr, cam_idx, xy, n_images, point_ok=point_ok)
    m = int(n_images)
    K, R, t = np.full((m, 3, 3), np.nan), np.full((m, 3, 3), np.nan), np.full((m, 3), np.nan)
    good = status == 0
    if good.any():
        K[good], R[good], t[good] = decompose_projection(P[good], f0)
    return K, R, t, {"status": status, "quality": quality, "P": P, "timings_ms": tm}
