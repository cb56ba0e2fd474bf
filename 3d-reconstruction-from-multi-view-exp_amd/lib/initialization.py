"""Initial estimates for bundle adjustment when visibility is sparse: triangulate every point from the cameras that
are known, resect every camera from the points that are known -- the two steps that extend a reconstruction.  Both run
on the MI355X (``mvba_triangulate``, ``mvba_resect``: csrc/mvba_init.h); there is no CPU fallback.

And the step that starts one: co-visibility counts and the fundamental matrix of two views from the points they share
(``mvba_covisibility``, ``mvba_two_view``: csrc/mvba_twoview.h), the relative pose out of it, and
``bootstrap``, the incremental driver -- host control flow over the device calls -- that grows a start pair into an
initial estimate for ``BundleAdjuster.from_observations``.  With wrong matches among the tracks the first F comes from 8-point
RANSAC on the device instead (``mvba_two_view_robust``: csrc/mvba_ransac.h): ``ransac_threshold``; and every
later camera from 6-point RANSAC (``mvba_resect_robust``: csrc/mvba_resect_ransac.h): ``resect_threshold``; and
every point from a two-view RANSAC of its own (``mvba_triangulate_robust``: csrc/mvba_tri_ransac.h):
``triangulate_threshold``.  With the intrinsics known -- ``bootstrap`` is given them -- a later camera is better registered by
its POSE alone: three-point RANSAC and a pose-only Gauss-Newton refit (``mvba_pose_robust``, ``mvba_pose_refine``:
csrc/mvba_pose_ransac.h): ``pose_threshold``.  A PLANAR scene has no fundamental matrix: its start pair comes from
4-point RANSAC for the homography (``mvba_homography_robust``: csrc/mvba_homography.h) and the decomposition of it:
``model``.

And the step that takes a reconstruction into another frame -- that of surveyed control points, or of a second map: the
similarity between two point sets by 3-point RANSAC and by least squares (``mvba_align_robust``, ``mvba_align``:
csrc/mvba_align.h): ``robust_similarity``, ``fit_similarity``, ``transform_reconstruction``,
``align_to_control_points``.

And the step in front of them all -- from what a matcher delivers, keypoints per image and matched keypoint pairs per image
pair, to the tracks (``pt_ptr``, ``cam_idx``, ``xy``) everything above takes: the connected components of the match graph on the
device (``mvba_build_tracks``: csrc/mvba_tracks.h): ``build_tracks``, with ``verify_matches`` -- the two-view RANSAC
above, pair by pair -- to mark the matches worth using.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from . import _mvba


def _confidence(out, count_key, sample_size, n_hypotheses):
    """1 - (1 - w^s)^H with w = n_inliers / ``out[count_key]``, the probability that one of H samples of s was all inliers; 0 where
    the status is not 0."""
    with np.errstate(all="ignore"):
        w = out["n_inliers"] / np.maximum(out[count_key], 1)
        return np.where(out["status"] == 0, 1.0 - (1.0 - w ** sample_size) ** int(n_hypotheses), 0.0)


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


def robust_triangulate_points(pt_ptr, cam_idx, xy, K, R, t, threshold, n_hypotheses: int = 64, seed: int = 0, n_refine: int = 2,
                              n_refit: int = 2):
    """(X (N, 3), info): ``triangulate_points`` by a two-view RANSAC per point on the device (``mvba_triangulate_robust``).  A
    hypothesis is two of the point's observations and its model the midpoint of their two viewing rays; a point with at most
    ``n_hypotheses`` pairs tries every pair, any other ``n_hypotheses`` sampled ones (a counter-based generator of ``seed``, the
    point and the hypothesis number: ``triangulate_sample``).  The score is the number of the point's observations in front of
    their camera whose reprojection distance is at most ``threshold`` (units of xy); the best hypothesis's inliers get the
    plain fit (the DLT, ``n_refine`` Gauss-Newton steps), ``n_refit`` times at most: the first is kept if it has min(deg, 3)
    inliers of its own, a later one while its inlier set does not shrink.  ``info``: ``status`` (N,) -- 0 ok, 1 fewer than two
    observations, 2 every hypothesis degenerate (no parallax), 4 the best hypothesis has fewer than min(deg, 3) inliers; X
    and quality are NaN where it is not 0 --, ``quality`` (N, 3) -- the three figures of ``triangulate_points`` over the final
    inliers --, ``n_inliers``, ``best`` (N,), ``inlier`` (n_obs,) bool in the order of the list, ``confidence`` (N,) -- 1 where
    every pair was tried, 1 - (1 - w^2)^H with w = n_inliers / deg where they were sampled, 0 where the status is not 0 -- and
    ``timings_ms``.  A point with three or more observations needs three that agree; a point with exactly TWO cannot be
    verified: its one hypothesis is its own two observations, and a wrong match among them passes whenever the two rays come
    within the threshold of each other.  Two calls with the same arguments return the same bits."""
    out = _mvba.triangulate_robust(K, R, t, pt_ptr, cam_idx, xy, threshold, n_hypotheses=n_hypotheses, seed=seed, n_refine=n_refine,
                                   n_refit=n_refit)
    X = out.pop("X")
    m = np.asarray(K).shape[0]
    deg = np.full(len(X), m, np.int64) if pt_ptr is None else np.diff(np.asarray(pt_ptr, np.int64))
    exhaustive = (out["status"] == 0) & (deg * (deg - 1) // 2 <= int(n_hypotheses))
    out["confidence"] = np.where(exhaustive, 1.0, _confidence({**out, "deg": deg}, "deg", 2, n_hypotheses))
    return X, out


def triangulate_sample(seed, point, h, deg, n_hypotheses: int = 64):
    """The two observation numbers (i < j, below ``deg``) that hypothesis ``h`` of point ``point`` is made of under ``seed``, or
    (-1, -1) where every pair fits into ``n_hypotheses`` and there is no pair ``h`` -- the host instance of the function the
    kernel runs."""
    return _mvba.triangulate_sample(seed, point, h, deg, n_hypotheses)


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


def robust_resect_cameras(X, pt_ptr, cam_idx, xy, n_images: int, threshold, f0: float = 1.0, point_ok=None, cameras=None,
                          n_hypotheses: int = 512, seed: int = 0, n_refit: int = 2):
    """(K, R, t, info): ``resect_cameras`` by 6-point RANSAC on the device (``mvba_resect_robust``), for the cameras listed in
    ``cameras`` (default: all; K, R, t and every per-camera entry of ``info`` are indexed by the position in it).  Per camera,
    ``n_hypotheses`` minimal samples of its usable observations (a counter-based generator of ``seed``, the camera and the
    hypothesis number: ``resect_sample``) are solved and scored by the number of usable observations in front of the camera
    whose reprojection distance is at most ``threshold`` (units of xy); the best hypothesis's inliers get the full normalised
    DLT, ``n_refit`` times at most: the first is kept if it has 6 inliers of its own, a later one while its inlier set does not
    shrink.  ``info``: ``status`` -- 0 ok, 1 fewer than 6 usable observations, 2 every hypothesis degenerate (e.g. coplanar
    points), 4 the best hypothesis has fewer than 6 inliers; K, R, t, P and quality are NaN where it is not 0 --, ``quality``
    (C, 2) -- RMS reprojection residual over the final inliers, lambda_1 / lambda_2 of the last kept refit --, ``P`` (C, 3, 4),
    ``n_usable``, ``n_inliers``, ``best`` (C,), ``inlier`` (n_obs,) bool in the order of the list -- the final inliers of the
    listed cameras of status 0 --, ``confidence`` (C,) = 1 - (1 - w^6)^H with w = n_inliers / n_usable, and ``timings_ms``.
    Two calls with the same arguments return the same bits."""
    out = _mvba.resect_robust(X, pt_ptr, cam_idx, xy, n_images, threshold, point_ok=point_ok, cameras=cameras, n_hypotheses=n_hypotheses,
                              seed=seed, n_refit=n_refit)
    P, status = out["P"], out["status"]
    nc = P.shape[0]
    K, R, t = np.full((nc, 3, 3), np.nan), np.full((nc, 3, 3), np.nan), np.full((nc, 3), np.nan)
    good = status == 0
    if good.any():
        K[good], R[good], t[good] = decompose_projection(P[good], f0)
    out["confidence"] = _confidence(out, "n_usable", 6, n_hypotheses)
    return K, R, t, out


def resect_sample(seed, k, h, n):
    """The 6 distinct indices below ``n`` (of a camera's usable observations in ascending point order) that hypothesis ``h`` of
    camera ``k`` draws under ``seed`` -- the host instance of the function the kernel runs."""
    return _mvba.resect_sample(seed, k, h, n)


def robust_pose_cameras(X, pt_ptr, cam_idx, xy, K, threshold, point_ok=None, cameras=None, n_hypotheses: int = 512, seed: int = 0,
                        n_refine: int = 5, n_refit: int = 2):
    """(R, t, info): the poses of cameras whose intrinsics ``K`` (m, 3, 3) are KNOWN, from the points X (N, 3) they see, by
    three-point RANSAC on the device (``mvba_pose_robust``), for the cameras listed in ``cameras`` (default: all; R, t and every
    per-camera entry of ``info`` are indexed by the position in it).  ``K`` projects to the units of ``xy``:
    ``engine_intrinsics(init_K)`` for raw image coordinates.  Per camera, ``n_hypotheses`` samples of four usable observations (a
    counter-based generator of ``seed``, the camera and the hypothesis number: ``pose_sample``): the first three give up to
    four poses (P3P), the fourth picks one; the score is the number of usable observations in front of the camera whose
    reprojection distance is at most ``threshold`` (units of xy).  The best hypothesis's inliers get ``n_refine`` Gauss-Newton
    steps on the reprojection error in the six pose unknowns, ``n_refit`` times at most, each kept while its inlier set does
    not shrink.  Unlike ``robust_resect_cameras`` it needs 4 observations, not 6, coplanar points are no degeneracy, and the
    pose belongs to the given K.  ``info``: ``status`` -- 0 ok, 1 fewer than 4 usable observations, 2 every hypothesis
    degenerate (e.g. collinear points), 4 the best hypothesis has fewer than 4 inliers; R, t and quality are NaN where it is not
    0 --, ``quality`` (C, 2) -- RMS reprojection residual over the final inliers, smallest relative Cholesky pivot of the last
    kept refit --, ``n_usable``, ``n_inliers``, ``best`` (C,), ``inlier`` (n_obs,) bool in the order of the list,
    ``confidence`` (C,) = 1 - (1 - w^4)^H with w = n_inliers / n_usable, and ``timings_ms``.  Two calls with the same arguments
    return the same bits."""
    out = _mvba.pose_robust(X, pt_ptr, cam_idx, xy, K, threshold, point_ok=point_ok, cameras=cameras, n_hypotheses=n_hypotheses, seed=seed,
                            n_refine=n_refine, n_refit=n_refit)
    R, t = out.pop("R"), out.pop("t")
    out["confidence"] = _confidence(out, "n_usable", 4, n_hypotheses)
    return R, t, out


def refine_poses(X, pt_ptr, cam_idx, xy, K, R, t, point_ok=None, obs_ok=None, cameras=None, n_steps: int = 10):
    """(R, t, info): the poses ``R`` (C, 3, 3), ``t`` (C, 3) of the listed cameras (default: all) refined against the FIXED
    points X by ``n_steps`` Gauss-Newton steps on the reprojection error (``mvba_pose_refine``: the refit of
    ``robust_pose_cameras`` alone, without a threshold), over the observations of usable points that ``obs_ok`` (n_obs,) marks
    (default: all of them).  A step that would raise the cost is not taken and ends the camera's iteration.  ``info``:
    ``status`` -- 0 ok, 1 fewer than 3 observations, 2 singular at the first step or an input that is not finite; such a camera
    keeps its input pose --, ``quality`` (C, 3) -- RMS reprojection residual before, after, steps taken --, ``n_usable`` and
    ``timings_ms``."""
    out = _mvba.pose_refine(X, pt_ptr, cam_idx, xy, K, R, t, point_ok=point_ok, obs_ok=obs_ok, cameras=cameras, n_steps=n_steps)
    return out.pop("R"), out.pop("t"), out


def pose_sample(seed, k, h, n):
    """The 4 distinct indices below ``n`` (of a camera's usable observations in ascending point order) that hypothesis ``h`` of
    camera ``k`` draws under ``seed`` -- the host instance of the function the kernel runs."""
    return _mvba.pose_sample(seed, k, h, n)


def covisibility(pt_ptr, cam_idx, n_images):
    """count (m, m) int64: count[k, l] = the number of points observed in both k and l, count[k, k] = camera k's observation
    count (``mvba_covisibility``)."""
    return _mvba.covisibility(pt_ptr, cam_idx, n_images)[0]


def fundamental_matrices(pt_ptr, cam_idx, xy, n_images, pairs):
    """(F (P, 3, 3), info) of the camera pairs ``pairs`` (P, 2) = (k, l) from the points each pair shares: the normalised
    8-point method (``mvba_two_view``): x_l^T F x_k = 0 with ``xy`` in any units -- F is for those units --, rank 2, Frobenius
    norm 1, largest-magnitude entry positive.  ``info``: ``status`` (P,) -- 0 ok, 1 fewer than 8 shared points, 2 degenerate
    (noise-free points in a plane, two cameras at one centre); F and quality are NaN where it is not 0 --, ``quality`` (P, 2) --
    RMS Sampson distance in units of xy, eigenvalue ratio lambda_1 / lambda_2 (small: well determined) --, ``n_shared`` (P,)
    and ``timings_ms``.  Every shared point enters the fit: a gross outlier moves F, and ``quality`` shows it;
    ``robust_fundamental_matrices`` is the fit that tolerates them."""
    F, quality, n_shared, status, tm = _mvba.two_view(pt_ptr, cam_idx, xy, n_images, pairs)
    return F, {"status": status, "quality": quality, "n_shared": n_shared, "timings_ms": tm}


def robust_fundamental_matrices(pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses: int = 512, seed: int = 0,
                                n_refit: int = 2, return_inliers: bool = True):
    """(F (P, 3, 3), info): ``fundamental_matrices`` by 8-point RANSAC on the device (``mvba_two_view_robust``).  Per pair,
    ``n_hypotheses`` minimal samples (a counter-based generator of ``seed``, the pair and the hypothesis number:
    ``ransac_sample``) are solved and scored by the number of shared points whose Sampson distance is at most ``threshold``
    (units of xy); the best hypothesis's inliers get the full normalised 8-point fit, ``n_refit`` times at most, each kept while
    its own inlier set does not shrink.  ``info``: ``status`` (P,) -- 0 ok, 1 fewer than 8 shared points, 2 every hypothesis
    degenerate, 4 the best hypothesis has fewer than 8 inliers; F and quality are NaN where it is not 0 --, ``n_shared``,
    ``n_inliers``, ``best`` (P,), ``quality`` (P, 2) -- RMS Sampson distance over the final inliers, lambda_1 / lambda_2 of the
    last kept refit --, ``inlier`` (P, N) bool (``return_inliers``; P x N bytes), ``confidence`` (P,) = 1 - (1 - w^8)^H with
    w = n_inliers / n_shared -- the probability that one of H samples was all inliers -- and ``timings_ms``.  Two calls with
    the same arguments return the same bits."""
    out = _mvba.two_view_robust(pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses=n_hypotheses, seed=seed, n_refit=n_refit,
                                return_inliers=return_inliers)
    F = out.pop("F")
    out["confidence"] = _confidence(out, "n_shared", 8, n_hypotheses)
    return F, out


def ransac_sample(seed, k, l, h, n):
    """The 8 distinct indices below ``n`` (of a pair's shared points in ascending point order) that hypothesis ``h`` of pair
    (k, l) draws under ``seed`` -- the host instance of the function the kernel runs."""
    return _mvba.ransac_sample(seed, k, l, h, n)


def robust_homographies(pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses: int = 512, seed: int = 0, n_refit: int = 2,
                        return_inliers: bool = True):
    """(H (P, 3, 3), info): the homography x_l ~ H x_k of each pair (k, l) by 4-point RANSAC on the device
    (``mvba_homography_robust``) -- the two-view model of points in a plane, where the fundamental matrix is not determined.
    Per pair, ``n_hypotheses`` samples of four shared points (``homography_sample``) are solved in closed form and scored by the
    number of shared points that transfer within ``threshold`` (units of xy) in BOTH directions with a positive third
    coordinate; the best hypothesis's inliers get the normalised DLT, ``n_refit`` times at most, each kept while its own inlier
    set does not shrink.  H is in the units of xy, |H| = 1, largest-magnitude entry positive.  ``info``: ``status`` (P,) -- 0 ok,
    1 fewer than 4 shared points, 2 every hypothesis degenerate (collinear points), 4 the best hypothesis has fewer than 4
    inliers; H and quality are NaN where it is not 0 --, ``n_shared``, ``n_inliers``, ``best`` (P,), ``quality`` (P, 2) -- RMS
    symmetric transfer distance over the final inliers, lambda_1 / lambda_2 of the last kept refit --, ``inlier`` (P, N) bool
    (``return_inliers``), ``hyp_count`` (P, H), ``confidence`` (P,) = 1 - (1 - w^4)^H with w = n_inliers / n_shared, and
    ``timings_ms``.  Two calls with the same arguments return the same bits."""
    out = _mvba.homography_robust(pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses=n_hypotheses, seed=seed, n_refit=n_refit,
                                  return_inliers=return_inliers, return_counts=True)
    H = out.pop("H")
    out["confidence"] = _confidence(out, "n_shared", 4, n_hypotheses)
    return H, out


def homography_sample(seed, k, l, h, n):
    """The 4 distinct indices below ``n`` (of a pair's shared points in ascending point order) that hypothesis ``h`` of pair
    (k, l) draws under ``seed`` -- the first four of ``ransac_sample`` wherever n >= 8; the host instance of the function the
    kernel runs."""
    return _mvba.homography_sample(seed, k, l, h, n)


def fit_similarity(src, dst, ok=None, with_scale: bool = True):
    """(s, Q, tau, info): the least-squares similarity ``dst ~ s Q src + tau`` of the rows ``ok`` allows whose six numbers are
    finite, on the device (``mvba_align``: csrc/mvba_align.h) -- Q a proper rotation, s = 1 with
    ``with_scale=False``.  ``info``: ``status`` (0 ok, 1 fewer than 3 usable rows, 2 src or dst on a line; s, Q, tau NaN where it
    is not 0), ``n_usable``, ``quality`` (RMS residual, relative gap of the two largest eigenvalues, mean squared spread of
    src).  One wrong row spoils it: ``robust_similarity``."""
    out = _mvba.align(src, dst, ok=ok, with_scale=with_scale)
    return out.pop("s"), out.pop("Q"), out.pop("tau"), out


def robust_similarity(src, dst, threshold, ok=None, with_scale: bool = True, n_hypotheses: int = 512, seed: int = 0, n_refit: int = 2):
    """(s, Q, tau, info): ``dst ~ s Q src + tau`` by 3-point RANSAC on the device (``mvba_align_robust``).  ``n_hypotheses``
    samples of three usable rows (``align_sample``) are solved by Horn's quaternion method and scored by the number of usable
    rows with ``|s Q x + tau - y| <= threshold`` (units of dst); the best hypothesis's inliers get the least-squares fit,
    ``n_refit`` times at most, the first kept if it has three inliers of its own, a later one while its set does not shrink.
    ``info``: ``status`` (0 ok, 1 fewer than 3 usable rows, 2 every hypothesis degenerate, 4 best count below 3), ``n_usable``,
    ``n_inliers``, ``best``, ``quality`` (3,), ``inlier`` (n,) bool, ``hyp_count`` (H,), ``confidence`` = 1 - (1 - w^3)^H with
    w = n_inliers / n_usable, and ``timings_ms``.  Two calls with the same arguments return the same bits."""
    out = _mvba.align_robust(src, dst, threshold, ok=ok, with_scale=with_scale, n_hypotheses=n_hypotheses, seed=seed, n_refit=n_refit,
                             return_counts=True)
    out["confidence"] = float(_confidence({k: np.asarray(out[k]) for k in ("n_inliers", "n_usable", "status")}, "n_usable", 3, n_hypotheses))
    return out.pop("s"), out.pop("Q"), out.pop("tau"), out


def align_sample(seed, h, n):
    """The 3 distinct indices below ``n`` (of the usable rows in ascending order) that hypothesis ``h`` draws under ``seed`` --
    the first three of ``ransac_sample(seed, 0, 0, h, n)`` wherever n >= 8; the host instance of the function the kernel runs."""
    return _mvba.align_sample(seed, h, n)


def transform_reconstruction(s, Q, tau, X=None, R=None, t=None):
    """(X', R', t'): a reconstruction under the similarity x -> s Q x + tau, in the camera convention K [R^T | -R^T t] (R is
    camera-to-world, t the centre): ``X' = s X Q^T + tau``, ``t' = s t Q^T + tau``, ``R' = Q R``.  Reprojections do not change.
    NaN rows stay NaN -- ``bootstrap``'s unreached cameras and points pass through --, an argument left out comes back None."""
    Q, tau = np.asarray(Q, np.float64), np.asarray(tau, np.float64)
    Xn = None if X is None else s * np.asarray(X, np.float64) @ Q.T + tau
    tn = None if t is None else s * np.asarray(t, np.float64) @ Q.T + tau
    Rn = None if R is None else Q @ np.asarray(R, np.float64)
    return Xn, Rn, tn


def align_to_control_points(X, R, t, point_ids, xyz, threshold, with_scale: bool = True, **search):
    """(X', R', t', info): the reconstruction in the frame of its control points.  ``xyz[i]`` is the surveyed position of point
    ``point_ids[i]``; ``robust_similarity`` runs from ``X[point_ids]`` to ``xyz`` (rows with a non-finite number are unusable;
    ``threshold`` in the units of xyz; ``search``: n_hypotheses, seed, n_refit) and ``transform_reconstruction`` applies it.
    ``info`` is ``robust_similarity``'s with ``s``, ``Q``, ``tau`` and ``held``: the point ids among the inliers, whose rows of X'
    are set to their surveyed xyz -- ready for ``BundleAdjuster.from_observations(..., init_X=X', hold_points=info["held"])``.
    Where the status is not 0 nothing is transformed: X, R, t come back as copies and ``held`` is empty."""
    ids, xyz = np.asarray(point_ids, np.int64).reshape(-1), np.asarray(xyz, np.float64).reshape(-1, 3)
    X, R, t = np.array(X, np.float64), np.array(R, np.float64), np.array(t, np.float64)
    assert len(ids) == len(xyz)
    s, Q, tau, info = robust_similarity(X[ids], xyz, threshold, with_scale=with_scale, **search)
    info.update(s=s, Q=Q, tau=tau, held=ids[info["inlier"]] if info["status"] == 0 else ids[:0])
    if info["status"] != 0:
        return X, R, t, info
    X, R, t = transform_reconstruction(s, Q, tau, X, R, t)
    X[ids[info["inlier"]]] = xyz[info["inlier"]]
    return X, R, t, info


def restrict_observations(pt_ptr, cam_idx, xy, point_ok, camera_ok):
    """The sub-list of the points and cameras marked: (pt_ptr, cam_idx, xy, point_ids, camera_ids) with points and cameras
    renumbered in ascending order of their old indices (``point_ids``, ``camera_ids``: the old index of each new one)."""
    pt_ptr, cam_idx = np.asarray(pt_ptr, np.int64), np.asarray(cam_idx, np.int32)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    point_ok, camera_ok = np.asarray(point_ok, bool), np.asarray(camera_ok, bool)
    point_ids, camera_ids = np.nonzero(point_ok)[0], np.nonzero(camera_ok)[0]
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    keep = point_ok[pt] & camera_ok[cam_idx]
    new_cam = np.cumsum(camera_ok) - 1
    new_pt = np.cumsum(point_ok) - 1
    ptr = np.zeros(len(point_ids) + 1, np.int64)
    np.cumsum(np.bincount(new_pt[pt[keep]], minlength=len(point_ids)), out=ptr[1:])
    return ptr, new_cam[cam_idx[keep]].astype(np.int32), xy[keep], point_ids, camera_ids


def pose_candidates(E):
    """The four (R (3, 3), t (3,)) of the second camera that an essential matrix allows, the first at the origin with identity
    pose: x_l ~ R^T (X - t), |t| = 1 (the conventions of ``_mvba.project``), from the SVD of E with both singular values set to
    their mean, in the order (R_a, +), (R_a, -), (R_b, +), (R_b, -)."""
    U, s, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    out = []
    for Rrel in (U @ W @ Vt, U @ W.T @ Vt):  # x_l ~ Rrel x_k + tau, tau = +-U[:, 2]
        for tau in (U[:, 2], -U[:, 2]):
            out.append((Rrel.T, -Rrel.T @ tau))
    return out


def homography_pose_candidates(Hn):
    """The four (R (3, 3), t (3,), n (3,)) that a calibrated homography ``Hn`` = K_l^-1 H K_k allows, in the conventions of
    ``pose_candidates`` (the first camera at the origin with identity pose, x_l ~ R^T (X - t), |t| = 1): Hn ~ R^T (I + t n^T / d) for
    points on the plane n . X = d of the first camera's frame; ``n`` comes back scaled by 1 / d, d in units of the baseline
    (|n| = 1 / d).  Hn is scaled so that its middle singular value is 1 and its determinant positive; the candidates come from
    the eigen-decomposition of Hn^T Hn (Faugeras and Lustman 1988, in the form of Ma, Soatto, Kosecka and Sastry 2004, 5.3): the
    two unit vectors u in span(v_1, v_3) whose length Hn keeps (every eigenvector with its largest component positive: the order
    of the list is defined), each with the rotation that takes (v_2, u, v_2 x u) to their images,
    in the order (R_a, +), (R_a, -), (R_b, +), (R_b, -) of (t, n)'s sign.  If sigma_1 - sigma_3 <= 1e-12 sigma_2 the homography
    is a rotation (no baseline, any plane): the list is empty."""
    Hn = np.asarray(Hn, np.float64)
    if not np.isfinite(Hn).all():
        return []
    sv = np.linalg.svd(Hn, compute_uv=False)
    if not sv[1] > 0 or sv[0] - sv[2] <= 1e-12 * sv[1]:
        return []
    Hn = Hn / sv[1] * (1.0 if np.linalg.det(Hn) > 0 else -1.0)
    w, V = np.linalg.eigh(Hn.T @ Hn)  # ascending: sigma_3^2, 1, sigma_1^2
    V = V * np.where(V[np.abs(V).argmax(axis=0), np.arange(3)] < 0, -1.0, 1.0)  # each eigenvector: largest component positive
    v1, v2, v3 = V[:, 2], V[:, 1], V[:, 0]
    s1, s3 = max(w[2], 1.0), min(w[0], 1.0)
    a, b = np.sqrt(1.0 - s3), np.sqrt(s1 - 1.0)
    out = []
    for u in ((a * v1 + b * v3) / np.sqrt(s1 - s3), (a * v1 - b * v3) / np.sqrt(s1 - s3)):
        U = np.stack([v2, u, np.cross(v2, u)], axis=1)
        W = np.stack([Hn @ v2, Hn @ u, np.cross(Hn @ v2, Hn @ u)], axis=1)
        Rrel, nn = W @ U.T, np.cross(v2, u)  # x_l ~ Rrel x_k + tau / d (n . x_k)
        tau = (Hn - Rrel) @ nn
        d = 1.0 / np.linalg.norm(tau)  # the plane's distance in units of the baseline
        t = -Rrel.T @ tau * d
        for sgn in (1.0, -1.0):
            out.append((Rrel.T, sgn * t, sgn * nn / d))
    return out


def _pair_candidates(pt_ptr, cam_idx, xy, K, k, l, cands, point_ok, n_used, n_refine):
    """The candidate selection both routes of ``relative_pose`` share.  ``cands``: four (R, t, ...) of camera l with camera k at the
    origin; ``point_ok`` (N,): the points to triangulate over (None: all); ``n_used``: the count "more than half" is measured
    against.  The two-camera sub-list is built once (the lower camera index becomes 0) and every candidate triangulated on the
    device without refinement: (n_front (4,) -- the points of status 0 and smallest depth > 0 --, rms (4,) -- the RMS reprojection
    residual of those points, inf where there are none --, take).  ``take(c, R, t, X, quality)``: False if candidate c does not
    put more than half of ``n_used`` in front of both cameras; otherwise it is triangulated again with ``n_refine`` and written
    into R (2, 3, 3), t (2, 3) and, for the points in front, into X and quality (N, 3)."""
    cam_ok = np.zeros(K.shape[0], bool)
    cam_ok[[k, l]] = True
    ptr, cam, z, ids, _ = restrict_observations(pt_ptr, cam_idx, xy, np.ones(len(pt_ptr) - 1, bool) if point_ok is None else point_ok, cam_ok)
    ik, il = (0, 1) if k < l else (1, 0)
    K2, R2, t2 = np.empty((2, 3, 3)), np.empty((2, 3, 3)), np.zeros((2, 3))
    K2[ik], K2[il], R2[ik] = K[k], K[l], np.eye(3)

    def tri(c, nr):
        R2[il], t2[il] = cands[c][:2]
        Xc, q, st, _ = _mvba.triangulate(K2, R2, t2, ptr, cam, z, n_refine=nr)
        return Xc, q, (st == 0) & (q[:, 1] > 0)

    n_front, rms = np.zeros(4, np.int64), np.full(4, np.inf)
    for c in range(4):
        _, q, front = tri(c, 0)
        n_front[c] = front.sum()
        if front.any():
            rms[c] = np.sqrt(np.mean(q[front, 0] ** 2))

    def take(c, R, t, X, quality):
        if not 2 * n_front[c] > n_used:
            return False
        Xc, q, front = tri(c, n_refine)
        X[ids[front]], quality[ids[front]] = Xc[front], q[front]
        R[0], t[0] = np.eye(3), 0.0
        R[1], t[1] = cands[c][:2]
        return True

    return n_front, rms, take


def relative_pose(pt_ptr, cam_idx, xy, K, pair, n_refine: int = 2, ransac_threshold=None, n_hypotheses: int = 512, seed: int = 0,
                  model: str = "fundamental", homography_threshold=None, planar_ratio: float = 0.8, _candidate=None, _fit=None):
    """(R (2, 3, 3), t (2, 3), X (N, 3), info): the pose of camera l = pair[1] relative to camera k = pair[0], which sits at the
    origin with identity pose; |t_l| = 1.  ``K`` (m, 3, 3) projects to the units of ``xy`` (raw image coordinates:
    ``engine_intrinsics(init_K)``, as for ``triangulate_points``).  F of the pair on the device, E = K_l^T F K_k, its four
    (R, +-t) candidates, each triangulated on the device without refinement; the winner has the most points of status 0 and
    smallest depth > 0, and is triangulated again with ``n_refine``.  ``X`` is NaN for points not shared, not triangulated or
    behind a camera.  ``info``: ``n_front`` (4,), ``status`` -- 0 ok, the ``fundamental_matrices`` status otherwise, 3 when no
    candidate puts more than half of the shared points in front of both cameras --, ``F``, ``n_shared``, ``two_view`` (the
    quality of F) and the triangulation ``quality`` (N, 3).
    With ``ransac_threshold`` (a Sampson distance in the units of xy) F is ``robust_fundamental_matrices``'s, with
    ``n_hypotheses`` and ``seed``; only the pair's inliers are triangulated -- the other shared points stay NaN in X --, "more
    than half" counts against the inliers, the status may also be 2 or 4 of that function, and ``info`` gains ``inlier`` (N,)
    bool and ``n_inliers``.
    ``model``: "fundamental" is all of the above.  "homography" is the start for a PLANAR scene (a wall, a floor, a document,
    flat ground from the air), where F is not determined and the route above returns a wrong pose without saying so: H of the
    pair by ``robust_homographies`` with ``homography_threshold`` (a transfer distance in the units of xy; default:
    ``ransac_threshold``; one of the two is needed), ``homography_pose_candidates(K_l^-1 H K_k)``, each triangulated on the device
    over the H inliers; the winner has the most points in front of both cameras, on a tie the lower RMS reprojection residual
    of those points, then the lower index.  "auto" (needs ``ransac_threshold``) runs both
    robust fits and takes the homography when n_inliers_H >= ``planar_ratio`` x n_inliers_F (a plane's points all fit one H, a
    general scene's do not: measured ratios >= 0.9 against <= 0.2), the route above otherwise.  ``info`` gains
    ``model`` (the one taken) and, where H was fitted, ``H``, ``n_inliers_H``; on the homography route also ``candidates`` (the
    list of (R, t, n)), ``plane`` (n, d: unit normal in camera k's frame and distance in units of the baseline),
    ``n_front`` and ``rms`` per candidate, ``best_candidate`` (the index taken), ``ambiguous`` -- True when a second candidate puts as many points in front: the data
    of two views cannot tell the two, ``bootstrap`` tries both -- and ``inlier``, ``n_inliers`` of H.  Status 3 is also returned
    when the candidate list is empty (a pure rotation); 1, 2, 4 are then ``robust_homographies``'s.
    (``_candidate`` and ``_fit`` are ``bootstrap``'s and this function's own: the index of the homography candidate to take instead
    of the winner, 0 .. 3, and the robust F fit "auto" has already made, so that the fundamental route does not repeat it.)"""
    K = np.asarray(K, np.float64)
    k, l = int(pair[0]), int(pair[1])
    n = len(pt_ptr) - 1
    if model not in ("fundamental", "homography", "auto"):
        raise ValueError(f"relative_pose: model = {model!r} must be 'fundamental', 'homography' or 'auto'")
    if model != "fundamental":
        thr_h = ransac_threshold if homography_threshold is None else homography_threshold
        if thr_h is None or (model == "auto" and ransac_threshold is None):
            raise ValueError(f"relative_pose: model = {model!r} needs ransac_threshold" + (" or homography_threshold" if model == "homography" else ""))
        Hm, hi = robust_homographies(pt_ptr, cam_idx, xy, K.shape[0], [(k, l)], thr_h, n_hypotheses=n_hypotheses, seed=seed)
        extra = {"H": Hm[0], "n_inliers_H": int(hi["n_inliers"][0])}
        if model == "auto":
            fit = robust_fundamental_matrices(pt_ptr, cam_idx, xy, K.shape[0], [(k, l)], ransac_threshold, n_hypotheses=n_hypotheses, seed=seed)
            fi = fit[1]
            extra["n_inliers_F"] = int(fi["n_inliers"][0])
            planar = hi["status"][0] == 0 and (fi["status"][0] != 0 or extra["n_inliers_H"] >= planar_ratio * extra["n_inliers_F"])
            if not planar:
                R, t, X, info = relative_pose(pt_ptr, cam_idx, xy, K, pair, n_refine, ransac_threshold, n_hypotheses, seed, _fit=fit)
                info.update(extra, model="fundamental")
                return R, t, X, info
        return _homography_pose(pt_ptr, cam_idx, xy, K, k, l, n_refine, Hm[0], hi, extra, _candidate)
    inlier = None
    if ransac_threshold is None:
        F, fi = fundamental_matrices(pt_ptr, cam_idx, xy, K.shape[0], [(k, l)])
    else:
        F, fi = _fit if _fit is not None else robust_fundamental_matrices(pt_ptr, cam_idx, xy, K.shape[0], [(k, l)], ransac_threshold,
                                                                          n_hypotheses=n_hypotheses, seed=seed)
        inlier = fi["inlier"][0]
    R, t, X = np.full((2, 3, 3), np.nan), np.full((2, 3), np.nan), np.full((n, 3), np.nan)
    info = {"n_front": np.zeros(4, np.int64), "status": int(fi["status"][0]), "F": F[0], "n_shared": int(fi["n_shared"][0]),
            "two_view": fi["quality"][0], "quality": np.full((n, 3), np.nan), "model": "fundamental"}
    n_used = info["n_shared"]
    if inlier is not None:
        info["inlier"], info["n_inliers"] = inlier, int(fi["n_inliers"][0])
        n_used = info["n_inliers"]
    if info["status"] != 0:
        return R, t, X, info
    info["n_front"], _, take = _pair_candidates(pt_ptr, cam_idx, xy, K, k, l, pose_candidates(K[l].T @ F[0] @ K[k]), inlier, n_used, n_refine)
    if not take(int(np.argmax(info["n_front"])), R, t, X, info["quality"]):
        info["status"] = 3
    return R, t, X, info


def _homography_pose(pt_ptr, cam_idx, xy, K, k, l, n_refine, H, hi, extra, candidate):
    """``relative_pose``'s homography route from the fitted H (``hi``: the info of ``robust_homographies`` for the one pair)."""
    n = len(pt_ptr) - 1
    R, t, X = np.full((2, 3, 3), np.nan), np.full((2, 3), np.nan), np.full((n, 3), np.nan)
    inlier = hi["inlier"][0]
    info = {"n_front": np.zeros(4, np.int64), "rms": np.full(4, np.inf), "status": int(hi["status"][0]), "F": np.full((3, 3), np.nan),
            "n_shared": int(hi["n_shared"][0]), "two_view": hi["quality"][0], "quality": np.full((n, 3), np.nan), "model": "homography",
            "inlier": inlier, "n_inliers": extra["n_inliers_H"], "candidates": [], "plane": None, "ambiguous": False, **extra}
    if info["status"] != 0:
        return R, t, X, info
    cands = homography_pose_candidates(np.linalg.solve(K[l], H) @ K[k])
    info["candidates"] = cands
    if not cands:
        info["status"] = 3
        return R, t, X, info
    info["n_front"], info["rms"], take = _pair_candidates(pt_ptr, cam_idx, xy, K, k, l, cands, inlier, info["n_inliers"], n_refine)
    best = min(range(4), key=lambda c: (-info["n_front"][c], info["rms"][c], c))
    info["ambiguous"] = bool((info["n_front"] >= info["n_front"][best]).sum() > 1)
    if candidate is not None:
        if not 0 <= int(candidate) < len(cands):
            raise ValueError(f"relative_pose: _candidate = {candidate} must be in 0 .. {len(cands) - 1}")
        best = int(candidate)
    if not take(best, R, t, X, info["quality"]):
        info["status"] = 3
        return R, t, X, info
    nn = cands[best][2]
    info["plane"] = (nn / np.linalg.norm(nn), 1.0 / np.linalg.norm(nn))
    info["best_candidate"] = best
    return R, t, X, info


def pose_for_intrinsics(P, K, c):
    """(R, t) of a camera with the GIVEN intrinsics ``K`` (3, 3; it projects to the units P projects to) that images the
    neighbourhood of the point ``c`` as the camera matrix ``P`` (3, 4) does: the rotation of ``decompose_projection``, and the
    centre moved along the ray of ``c`` so that ``c`` keeps its image and its magnification f / depth.  The centre of P itself
    belongs to P's own focal length -- the DLT trades the two against each other, a few percent at a noise of 1e-3 --, and
    taken with another K it is off by that factor of the depth."""
    Kd, R, td = decompose_projection(P, 1.0)
    y = R.T @ (np.asarray(c, np.float64) - td)  # c in P's camera frame
    x = Kd[0, 0] * y[:2] / y[2] + Kd[:2, 2]  # its image
    d = y[2] * K[0, 0] / Kd[0, 0]
    return R, c - R @ (d * np.array([(x[0] - K[0, 2]) / K[0, 0], (x[1] - K[1, 2]) / K[1, 1], 1.0]))


def _usable_counts(pt_ptr, cam_idx, point_ok, n_images):
    """(m,) the observations each camera has of the points marked."""
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    return np.bincount(np.asarray(cam_idx)[np.asarray(point_ok, bool)[pt]], minlength=n_images)


def _registration_count(status, count, min_points):
    """What a registration round of ``bootstrap`` would take: the largest ``count`` (inliers, or usable observations in the plain
    form) among the cameras of status 0 that have at least ``min_points``; 0 if there is none."""
    i = _registration_pick(status, count, min_points)
    return 0 if i is None else int(np.asarray(count)[i])


def _registration_pick(status, count, min_points):
    """The selection rule of a registration round: the index of the largest ``count`` among the cameras of status 0 that have at
    least ``min_points``, the lowest on ties; None if there is none."""
    status, count = np.asarray(status), np.asarray(count)
    good = (status == 0) & (count >= min_points)
    return int(np.argmax(np.where(good, count, -1))) if good.any() else None


# The registration step of ``bootstrap`` in its three forms, one signature: (X, point_ok, camera_ok, s) with ``s`` the constant
# inputs -> None when no unregistered camera qualifies, otherwise (c, R_c, t_c, sel, count): the camera, its pose, the (n_obs,)
# mask of the observations it was registered from, and the count that ranked it.
def _register_plain(X, point_ok, camera_ok, s):
    """``resect_cameras``; ranked by usable observations, registered from all of them."""
    todo = np.nonzero(~camera_ok)[0]
    ri = resect_cameras(X, s.pt_ptr, s.cam_idx, s.xy, s.m, f0=s.f0, point_ok=point_ok)[3]
    usable = _usable_counts(s.pt_ptr, s.cam_idx, point_ok, s.m)[todo]
    i = _registration_pick(ri["status"][todo], usable, s.min_points)
    if i is None:
        return None
    c = int(todo[i])
    sel = point_ok[s.pt] & (s.cam_idx == c)
    return (c, *pose_for_intrinsics(ri["P"][c], s.Kxy[c], X[s.pt[sel]].mean(axis=0)), sel, int(usable[i]))


def _register_resect(X, point_ok, camera_ok, s):
    """``robust_resect_cameras`` on the unregistered cameras (``resect_threshold``); ranked by inliers, registered from them."""
    todo = np.nonzero(~camera_ok)[0]
    ri = robust_resect_cameras(X, s.pt_ptr, s.cam_idx, s.xy, s.m, s.threshold, f0=s.f0, point_ok=point_ok, cameras=todo,
                               n_hypotheses=s.n_hypotheses, seed=s.seed)[3]
    i = _registration_pick(ri["status"], ri["n_inliers"], s.min_points)
    if i is None:
        return None
    c = int(todo[i])
    sel = ri["inlier"] & (s.cam_idx == c)
    return (c, *pose_for_intrinsics(ri["P"][i], s.Kxy[c], X[s.pt[sel]].mean(axis=0)), sel, int(ri["n_inliers"][i]))


def _register_pose(X, point_ok, camera_ok, s):
    """``robust_pose_cameras`` on the unregistered cameras (``pose_threshold``); ranked by inliers, the pose taken as returned."""
    todo = np.nonzero(~camera_ok)[0]
    Rp, tp, ri = robust_pose_cameras(X, s.pt_ptr, s.cam_idx, s.xy, s.Kxy, s.threshold, point_ok=point_ok, cameras=todo,
                                     n_hypotheses=s.n_hypotheses, seed=s.seed)
    i = _registration_pick(ri["status"], ri["n_inliers"], s.min_points)
    if i is None:
        return None
    c = int(todo[i])
    return c, Rp[i], tp[i], ri["inlier"] & (s.cam_idx == c), int(ri["n_inliers"][i])


def _other_start_wins(first, other, other_status):
    """``bootstrap`` with an ambiguous start pair: the second candidate replaces the first only if it was triangulated (status 0)
    and the camera registered from its points has MORE inliers; a tie keeps the first."""
    return other_status == 0 and other > first


def _kept_list(pt_ptr, cam_idx, xy, obs_ok, camera_ok):
    """``restrict_observations`` over all points and the cameras marked, without the observations ``obs_ok`` drops: (pt_ptr,
    cam_idx, xy, camera_ids)."""
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    keep = obs_ok & camera_ok[cam_idx]
    ptr = np.zeros(len(pt_ptr), np.int64)
    np.cumsum(np.bincount(pt[keep], minlength=len(pt_ptr) - 1), out=ptr[1:])
    return ptr, (np.cumsum(camera_ok) - 1)[cam_idx[keep]].astype(np.int32), xy[keep], np.nonzero(camera_ok)[0]


def bootstrap(pt_ptr, cam_idx, xy, init_K, f0: float = 1.0, start_pair=None, min_points: int = 12, max_rms=None, ransac_threshold=None,
              n_hypotheses: int = 512, seed: int = 0, resect_threshold=None, triangulate_threshold=None, pose_threshold=None,
              model: str = "fundamental", homography_threshold=None, planar_ratio: float = 0.8):
    """(K, R, t, X, info): an initial estimate for ``BundleAdjuster.from_observations`` from feature tracks and rough
    intrinsics, by incremental reconstruction.  ``xy`` are raw image coordinates, ``init_K`` (m, 3, 3) the adjuster's
    [[f,0,u],[0,f,v],[0,0,f0]]; K comes back as ``init_K`` (no focal length is estimated).
    Start pair (unless given): of the pairs in descending co-visibility, the first 16 with at least 8 shared points get
    ``relative_pose``; the one with the largest median ray angle among those of status 0 starts.  Then, until no camera can
    be added: ``resect_cameras`` on the current points; the unregistered camera with the most usable observations is
    registered if its status is 0 and it has at least ``min_points`` -- its pose only, the one that belongs to ``init_K``
    (``pose_for_intrinsics`` at the centroid of the points it sees) --; ``triangulate_points`` over the
    registered cameras; a point is kept if its status is 0, its smallest depth > 0 and, with ``max_rms``, its RMS residual
    (units of xy) is at most that.  No BA runs in between.  ``ransac_threshold``, ``n_hypotheses`` and ``seed`` go to every
    ``relative_pose`` (a robust first F; resection and triangulation stay as they are: ``max_rms`` is the filter there).
    With ``resect_threshold`` (a reprojection distance in the units of xy) each round runs ``robust_resect_cameras`` on the
    unregistered cameras instead, with ``n_hypotheses`` and ``seed``: the candidate is the one with the most inliers (status 0,
    at least ``min_points`` of them, the lowest index on ties), its pose is ``pose_for_intrinsics`` at the centroid of its inlier
    points, and its usable observations that are not inliers are dropped from every later triangulation and resection;
    ``info`` gains ``obs_ok`` (n_obs,) bool, the observations still in use, and ``inlier`` (n_obs,) bool, the observations
    the registered cameras were resected from.
    With ``pose_threshold`` (a reprojection distance in the units of xy) each round runs ``robust_pose_cameras`` on the
    unregistered cameras with ``engine_intrinsics(init_K)`` instead: the calibrated form of the same step.  The candidate rule,
    the dropping of usable observations that are not inliers, ``info["obs_ok"]`` and ``info["inlier"]`` are those of
    ``resect_threshold``; the pose is taken as returned (it already belongs to ``init_K``: no ``pose_for_intrinsics``).  Giving
    both thresholds is a ValueError.
    With ``triangulate_threshold`` (a reprojection distance in the units of xy) every triangulation of the loop is
    ``robust_triangulate_points`` over the observations of the registered cameras still in use, with ``n_hypotheses`` (4096 at
    most) and ``seed``: a wrong match in ANY registered camera, 0 and 1 included, is left out of its point instead of moving it
    (a point seen twice cannot be verified, see there).  The keep rule is the same (status 0, smallest depth > 0, ``max_rms``
    over the point's inliers).  Triangulation drops nothing for good: each round decides again over the cameras registered
    then.  ``relative_pose``'s own triangulation stays plain (two views have no redundancy).  ``info`` gains ``tri_inlier``
    (n_obs,) bool, the observations the final points were triangulated from.
    ``model``, ``homography_threshold`` and ``planar_ratio`` go to every ``relative_pose``: "homography" or "auto" start a planar
    scene from H.  Where the winning pair's two-view data cannot tell two pose candidates apart (``ambiguous``), the first
    registration round is run under each of the two, and the one whose registered camera has more inliers (more usable
    observations without a robust registration) starts; the first on a tie.  ``info`` gains ``model``, the one the start pair took.
    The output frame: camera 0 at the origin with identity pose, |t_1 - t_0| = 1.  ``info``: ``axis`` -- the gauge axis name
    whose component of t_1 is larger in magnitude: pass it to ``BundleAdjuster`` --, ``camera_ok`` (m,), ``point_ok`` (N,),
    ``order`` (the registration order), ``start_pair``.  Cameras and points not reached are NaN (``restrict_observations``
    gives the list without them).  ValueError if no start pair has status 0, or if camera 0 or 1 could not be registered."""
    if pose_threshold is not None and resect_threshold is not None:
        raise ValueError("bootstrap: pose_threshold and resect_threshold are two forms of one step: give one of them")
    pt_ptr, cam_idx = np.asarray(pt_ptr, np.int64), np.asarray(cam_idx, np.int32)
    xy, init_K = np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(init_K, np.float64)
    m, n = init_K.shape[0], len(pt_ptr) - 1
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    Kxy = engine_intrinsics(init_K)
    drops = resect_threshold is not None or pose_threshold is not None  # (a robust registration drops observations for good)
    register = _register_pose if pose_threshold is not None else _register_resect if resect_threshold is not None else _register_plain
    s = SimpleNamespace(pt_ptr=pt_ptr, cam_idx=cam_idx, xy=xy, pt=pt, m=m, Kxy=Kxy, f0=f0, min_points=min_points, n_hypotheses=n_hypotheses,
                        seed=seed, threshold=pose_threshold if pose_threshold is not None else resect_threshold)
    start = dict(ransac_threshold=ransac_threshold, n_hypotheses=n_hypotheses, seed=seed, model=model, homography_threshold=homography_threshold,
                 planar_ratio=planar_ratio)
    if start_pair is None:
        count = covisibility(pt_ptr, cam_idx, m)
        ks, ls = np.triu_indices(m, 1)
        order = np.argsort(-count[ks, ls], kind="stable")
        tried = [(int(ks[i]), int(ls[i])) for i in order if count[ks[i], ls[i]] >= 8][:16]
    else:
        tried = [(int(start_pair[0]), int(start_pair[1]))]
    best = None
    for pair in tried:
        R2, t2, X2, pi = relative_pose(pt_ptr, cam_idx, xy, Kxy, pair, **start)
        if pi["status"] != 0:
            continue
        angle = float(np.nanmedian(pi["quality"][:, 2]))
        if best is None or angle > best[0]:
            best = (angle, pair, R2, t2, X2, pi)
    if best is None:
        raise ValueError(f"bootstrap: no start pair with status 0 among {tried}")
    _, pair, R2, t2, X, pi = best
    camera_ok = np.zeros(m, bool)
    camera_ok[list(pair)] = True
    if pi.get("ambiguous"):  # two views of a plane allow two poses: the third camera decides
        nf = pi["n_front"]
        other = [c for c in range(4) if c != pi["best_candidate"] and nf[c] >= nf[pi["best_candidate"]]][0]
        Ro, to, Xo, po = relative_pose(pt_ptr, cam_idx, xy, Kxy, pair, **{**start, "model": "homography"}, _candidate=other)
        # the count (inliers, usable observations) of the camera the first registration round would take from each start's points
        first, second = (None if camera_ok.all() else register(Xc, np.isfinite(Xc).all(axis=1), camera_ok, s) for Xc in (X, Xo))
        if _other_start_wins(0 if first is None else first[4], 0 if second is None else second[4], po["status"]):
            R2, t2, X, pi = Ro, to, Xo, po
    R, t = np.full((m, 3, 3), np.nan), np.full((m, 3), np.nan)
    R[list(pair)], t[list(pair)] = R2, t2
    point_ok = np.isfinite(X).all(axis=1)
    reg_order = [pair[0], pair[1]]
    obs_ok, inlier = np.ones(len(cam_idx), bool), np.zeros(len(cam_idx), bool)  # (all in use until a robust registration drops some)
    tri_inlier = point_ok[pt] & camera_ok[cam_idx]  # (until the first round: what relative_pose triangulated from)
    while not camera_ok.all():
        reg = register(X, point_ok, camera_ok, s)
        if reg is None:
            break
        c, R[c], t[c], sel, _ = reg
        obs_ok &= ~((cam_idx == c) & point_ok[pt] & ~sel)  # (its usable observations it was not registered from: none in the plain form)
        inlier |= sel
        camera_ok[c] = True
        reg_order.append(c)
        ptr, cam, z, ids = _kept_list(pt_ptr, cam_idx, xy, obs_ok, camera_ok)
        if triangulate_threshold is None:
            X, ti = triangulate_points(ptr, cam, z, Kxy[ids], R[ids], t[ids])
        else:
            X, ti = robust_triangulate_points(ptr, cam, z, Kxy[ids], R[ids], t[ids], triangulate_threshold,
                                              n_hypotheses=min(int(n_hypotheses), 4096), seed=seed)
        point_ok = (ti["status"] == 0) & (ti["quality"][:, 1] > 0)
        if max_rms is not None:
            point_ok &= ti["quality"][:, 0] <= max_rms
        X[~point_ok] = np.nan
        if triangulate_threshold is not None:
            tri_inlier = np.zeros(len(cam_idx), bool)
            tri_inlier[np.nonzero(obs_ok & camera_ok[cam_idx])[0]] = ti["inlier"]  # (the list just triangulated)
            tri_inlier &= point_ok[pt]
    for c in (0, 1):
        if not camera_ok[c]:
            raise ValueError(f"bootstrap: camera {c} could not be registered (the output frame is that of cameras 0 and 1); "
                             f"registered: {reg_order}")
    R0, t0, scale = R[0].copy(), t[0].copy(), np.linalg.norm(t[1] - t[0])
    X, R, t = ((X - t0) @ R0) / scale, R0.T @ R, ((t - t0) @ R0) / scale
    axis = "x-right_z-forward" if abs(t[1, 0]) >= abs(t[1, 1]) else "x-up_z-forward"
    info = {"axis": axis, "camera_ok": camera_ok, "point_ok": point_ok, "order": reg_order, "start_pair": pair, "model": pi["model"]}
    if drops:
        info["obs_ok"], info["inlier"] = obs_ok, inlier
    if triangulate_threshold is not None:
        info["tri_inlier"] = tri_inlier
    return init_K.copy(), R, t, X, info


# ---- feature tracks from pairwise matches ----------------------------------------------------------------
def match_graph(keypoints, matches):
    """(kp_ptr (m + 1,) int64, kp_xy (n_nodes, 2), edges (M, 2) int32, image_pairs (M, 2), kp_pairs (M, 2)) of a matcher's output, as
    ``mvba_build_tracks`` takes it: keypoint j of image i is node ``kp_ptr[i] + j``.  ``keypoints``: a list of (n_i, 2) arrays, or the
    tuple ``(kp_ptr, kp_xy)``.  ``matches``: a dict ``{(k, l): (n, 2) int array}`` of keypoint indices local to images k and l --
    its matches are numbered in the dict's order --, or the tuple ``(image_pairs (M, 2), kp_pairs (M, 2))``.  ValueError for an
    image or a keypoint index out of range, with the match named."""
    if isinstance(keypoints, tuple) and len(keypoints) == 2 and np.ndim(keypoints[0]) == 1:
        kp_ptr, kp_xy = np.asarray(keypoints[0], np.int64), np.asarray(keypoints[1], np.float64).reshape(-1, 2)
    else:
        arrays = [np.asarray(a, np.float64).reshape(-1, 2) for a in keypoints]
        kp_ptr = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)
        kp_xy = np.concatenate(arrays) if arrays else np.zeros((0, 2))
    m = len(kp_ptr) - 1
    if m < 1 or kp_ptr[0] != 0 or (np.diff(kp_ptr) < 0).any() or kp_ptr[-1] != len(kp_xy):
        raise ValueError(f"match_graph: kp_ptr must ascend from 0 to the {len(kp_xy)} keypoints given, over at least one image")
    if isinstance(matches, dict):
        image_pairs = np.array([kl for kl, idx in matches.items() for _ in range(len(idx))], np.int64).reshape(-1, 2)
        kp_pairs = np.concatenate([np.asarray(idx, np.int64).reshape(-1, 2) for idx in matches.values()] + [np.zeros((0, 2), np.int64)])
    else:
        image_pairs, kp_pairs = (np.asarray(a, np.int64).reshape(-1, 2) for a in matches)
        if len(image_pairs) != len(kp_pairs):
            raise ValueError(f"match_graph: {len(image_pairs)} image pairs for {len(kp_pairs)} keypoint pairs")
    bad = np.nonzero(((image_pairs < 0) | (image_pairs >= m)).any(axis=1))[0]
    if len(bad):
        raise ValueError(f"match_graph: match {bad[0]} is between images {tuple(image_pairs[bad[0]].tolist())}: image index out of range, n_images = {m}")
    count = np.diff(kp_ptr)[image_pairs]
    bad = np.nonzero(((kp_pairs < 0) | (kp_pairs >= count)).any(axis=1))[0]
    if len(bad):
        raise ValueError(f"match_graph: match {bad[0]} joins keypoints {tuple(kp_pairs[bad[0]].tolist())} of images {tuple(image_pairs[bad[0]].tolist())}, "
                         f"which have {tuple(count[bad[0]].tolist())} keypoints")
    return kp_ptr, kp_xy, (kp_ptr[image_pairs] + kp_pairs).astype(np.int32), image_pairs, kp_pairs


def _flat_match_mask(matches, match_ok, n_matches):
    """``match_ok`` in the form of ``matches`` (a dict with its keys, or (M,)) as one (M,) bool array in the order of its matches."""
    if match_ok is None:
        return None
    if isinstance(match_ok, dict):
        if not isinstance(matches, dict) or set(match_ok) != set(matches):
            raise ValueError("build_tracks: a dict match_ok must have the keys of the dict matches")
        match_ok = np.concatenate([np.asarray(match_ok[kl]).reshape(-1) for kl in matches] + [np.zeros(0, bool)])
    match_ok = np.asarray(match_ok).reshape(-1) != 0
    if len(match_ok) != n_matches:
        raise ValueError(f"build_tracks: match_ok has {len(match_ok)} entries for {n_matches} matches")
    return match_ok


def build_tracks(keypoints, matches, min_length: int = 2, match_ok=None):
    """(pt_ptr, cam_idx, xy, info): feature tracks from pairwise matches, on the device (``mvba_build_tracks``) -- the list that
    ``covisibility``, ``bootstrap`` and ``BundleAdjuster.from_observations`` take as it is.  ``keypoints`` and ``matches`` as for
    ``match_graph``; ``match_ok`` marks the matches to use, in the form of ``matches`` (a dict with the same keys, or (M,); what
    ``verify_matches`` returns).  A track is a connected component of the match graph of at least ``min_length`` keypoints with at
    most one keypoint per image; a component with two keypoints of one image is dropped WHOLE (it is neither pruned nor
    split), and so is one with more keypoints than there are images, which cannot be otherwise.  Tracks are numbered in ascending
    order of their first keypoint (image-major), cameras ascend within a track, ``xy`` are the keypoints' coordinates, bit for bit.
    ``info``: ``kp_idx`` (n_obs,) -- the keypoint of each observation, local to its image --, ``obs_node``, ``node_track``
    (n_nodes,) -- >= 0 the keypoint's track, -1 unmatched, -2 its component is shorter than ``min_length``, -3 its component
    conflicts or is oversize --, ``kp_ptr``, the counts ``n_tracks``, ``n_obs``, ``n_components``, ``n_short``, ``n_conflicting``,
    ``n_conflicting_nodes``, ``n_oversize``, ``n_oversize_nodes``, ``n_singletons``, ``n_rounds`` (label rounds run) and
    ``timings_ms`` (upload, labels, layout, download).  The result is a function of the SET of matches used: their order, their
    orientation and duplicates change no bit of it, nor does a second call.  Limits: fewer than 2^31 keypoints in all."""
    kp_ptr, kp_xy, edges, _, _ = match_graph(keypoints, matches)
    out = _mvba.build_tracks(kp_ptr, kp_xy, edges, edge_ok=_flat_match_mask(matches, match_ok, len(edges)), min_length=min_length)
    pt_ptr, cam_idx, xy = out.pop("pt_ptr"), out.pop("cam_idx"), out.pop("xy")
    out["kp_idx"] = (out["obs_node"] - kp_ptr[cam_idx]).astype(np.int64)
    out["kp_ptr"] = kp_ptr
    return pt_ptr, cam_idx, xy, out


def match_pair_lists(keypoints, matches):
    """The matches of every image pair as a two-camera observation list, one "point" per match with its two observations in
    cameras k < l (a match given as (l, k) is turned round; a match inside one image belongs to no pair).  Returns ``(pairs (P, 2)
    ascending, lists, n_matches)``: ``lists[p] = (match ids (n,), pt_ptr (n + 1,), cam_idx (2 n,), xy (2 n, 2))`` with the ids in
    the numbering of ``match_graph``."""
    kp_ptr, kp_xy, edges, image_pairs, _ = match_graph(keypoints, matches)
    turn = image_pairs[:, 0] > image_pairs[:, 1]
    kl = np.where(turn[:, None], image_pairs[:, ::-1], image_pairs)
    nodes = np.where(turn[:, None], edges[:, ::-1], edges)
    ids = np.nonzero(kl[:, 0] != kl[:, 1])[0]
    pairs, which = np.unique(kl[ids], axis=0, return_inverse=True)
    which = which.reshape(-1)
    lists = []
    for p in range(len(pairs)):
        sel = ids[which == p]
        lists.append((sel, 2 * np.arange(len(sel) + 1, dtype=np.int64), np.tile(pairs[p].astype(np.int32), len(sel)), kp_xy[nodes[sel].reshape(-1)]))
    return pairs.reshape(-1, 2), lists, len(edges)


def verify_matches(keypoints, matches, threshold, model: str = "fundamental", n_hypotheses: int = 512, seed: int = 0):
    """(match_ok, info): the matches that agree with a two-view model of their image pair, found by RANSAC on the device -- glue
    over ``robust_fundamental_matrices`` (``model="fundamental"``: ``threshold`` is a Sampson distance) or ``robust_homographies``
    ("homography": a transfer distance, both ways), in the units of the keypoints.  Per image pair the pair's matches become a
    two-camera list (``match_pair_lists``) and the model's inlier mask comes back per match; a pair whose status is not 0 (too few
    matches, every sample degenerate) keeps none, nor does a match inside one image.  ``match_ok`` has the form of ``matches`` (a
    dict with its keys, or (M,) bool) and goes to ``build_tracks(match_ok=)``.  ``info``: ``pairs`` (P, 2), ``status``,
    ``n_matches``, ``n_inliers`` (P,), ``model`` (P, 3, 3).  Limit: ONE device call per image pair, which keeps the (P, N) inlier
    mask of the robust fits at one row -- thousands of pairs are thousands of small calls; and the camera cap of those fits."""
    if model not in ("fundamental", "homography"):
        raise ValueError(f"verify_matches: model must be 'fundamental' or 'homography', got {model!r}")
    fit = robust_fundamental_matrices if model == "fundamental" else robust_homographies
    pairs, lists, n_matches = match_pair_lists(keypoints, matches)
    m = len(match_graph(keypoints, matches)[0]) - 1
    ok = np.zeros(n_matches, bool)
    P = len(pairs)
    status, n_in, models = np.zeros(P, np.int32), np.zeros(P, np.int64), np.full((P, 3, 3), np.nan)
    for p, (ids, ptr, cam, xy) in enumerate(lists):
        M, fi = fit(ptr, cam, xy, m, pairs[p:p + 1], threshold, n_hypotheses=n_hypotheses, seed=seed)
        status[p], models[p] = fi["status"][0], M[0]
        if status[p] == 0:
            ok[ids] = fi["inlier"][0]
            n_in[p] = fi["n_inliers"][0]
    info = {"pairs": pairs, "status": status, "n_matches": np.array([len(l[0]) for l in lists], np.int64), "n_inliers": n_in, "model": models}
    if isinstance(matches, dict):
        cut = np.cumsum([len(v) for v in matches.values()])[:-1]
        return dict(zip(matches, np.split(ok, cut))), info
    return ok, info


# ---- the matches themselves, from uint8 descriptors ------------------------------------------------------
def descriptor_arrays(descriptors):
    """(kp_ptr (m + 1,) int64, desc (n_nodes, dim) uint8) of ``descriptors``: a list of (n_i, dim) uint8 arrays, or the tuple
    ``(kp_ptr, desc)``.  ValueError for a dtype other than uint8 -- nothing is cast silently --, for arrays of different ``dim`` and
    for a kp_ptr that does not ascend from 0 to the rows given."""
    def check(a, what):
        a = np.asarray(a)
        if a.dtype != np.uint8:
            raise ValueError(f"match_descriptors: {what} has dtype {a.dtype}; descriptors must be uint8.  Quantise them yourself, as the SIFT "
                             f"convention does for unit-norm floats: np.clip(np.rint(512 * d), 0, 255).astype(np.uint8)")
        if a.ndim != 2:
            raise ValueError(f"match_descriptors: {what} has shape {a.shape}; must be (n, dim)")
        return a
    if isinstance(descriptors, tuple) and len(descriptors) == 2 and np.ndim(descriptors[0]) == 1:
        kp_ptr, desc = np.asarray(descriptors[0], np.int64), check(descriptors[1], "desc")
    else:
        arrays = [check(a, f"descriptors[{i}]") for i, a in enumerate(descriptors)]
        dims = sorted({a.shape[1] for a in arrays})
        if len(dims) > 1:
            raise ValueError(f"match_descriptors: the images' descriptors have different dim: {dims}")
        kp_ptr = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)
        desc = np.concatenate(arrays) if arrays else np.zeros((0, 128), np.uint8)
    if len(kp_ptr) < 2 or kp_ptr[0] != 0 or (np.diff(kp_ptr) < 0).any() or kp_ptr[-1] != len(desc):
        raise ValueError(f"match_descriptors: kp_ptr must ascend from 0 to the {len(desc)} descriptors given, over at least one image")
    return kp_ptr, np.ascontiguousarray(desc)


def match_descriptors(descriptors, pairs=None, ratio=0.8, mutual: bool = True, max_distance=None, return_nn: bool = False):
    """(matches, info): keypoint matches from uint8 descriptors, by brute force on the device (``mvba_match_descriptors``; the i8
    matrix cores give every squared distance exactly).  ``descriptors`` as for ``descriptor_arrays``; ``pairs`` (P, 2) of (query
    image k, candidate image l), None for every k < l.  For every keypoint a of k: its nearest candidate b in l by (squared
    distance, index) -- a tie goes to the smaller index -- is its match unless, the first that holds: l has no keypoint; the
    distance exceeds ``max_distance`` (descriptor units; None: no test); with ``ratio`` (None: no test) NOT d2_best < ratio^2
    d2_second, or there is no second; with ``mutual`` the nearest keypoint of k to b is not a.  ``matches``: the dict ``{(k, l): (n, 2)
    int64}`` that ``verify_matches``, ``match_graph`` and ``build_tracks`` take, keys in the order of ``pairs``, rows by ascending a.
    ``info``: ``pairs``, ``distance2`` (the same keys: (n,) squared distances), ``n_matches``, ``n_queries``, ``n_no_candidate``,
    ``n_far``, ``n_ambiguous``, ``n_not_mutual``, ``timings_ms``; with ``return_nn`` ``nn_best``, ``nn_distance2``,
    ``nn_second2`` (the same keys: per query, before any test; -1 where there is none).  Integers throughout: the result is a
    function of the input alone, bit for bit.  Limits: uint8 only, dim a multiple of 16 up to 512; brute force; the ratio is
    tested in the forward direction only; a pair (l, k) is answered as given, and listing a pair twice is a ValueError here."""
    kp_ptr, desc = descriptor_arrays(descriptors)
    m = len(kp_ptr) - 1
    if pairs is None:
        pairs = [(k, l) for k in range(m) for l in range(k + 1, m)]
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    keys = [(int(k), int(l)) for k, l in pairs]
    if len(set(keys)) != len(keys):
        dup = next(kl for i, kl in enumerate(keys) if kl in keys[:i])
        raise ValueError(f"match_descriptors: pair {dup} is listed twice; the dict of matches cannot hold it")
    if ratio is not None and not 0.0 < float(ratio) <= 1.0:
        raise ValueError(f"match_descriptors: ratio = {ratio} must be in (0, 1], or None for no ratio test")
    if max_distance is not None and not float(max_distance) >= 0.0:
        raise ValueError(f"match_descriptors: max_distance = {max_distance} must be >= 0, or None for no distance test")
    max_dist2 = -1 if max_distance is None else int(min(np.floor(float(max_distance) ** 2), 2.0 ** 62))
    out = _mvba.match_descriptors(kp_ptr, desc, pairs, ratio=0.0 if ratio is None else float(ratio), mutual=mutual, max_dist2=max_dist2,
                                  want_nn=return_nn)
    ptr = out["match_ptr"]
    matches = {kl: out["kp_pairs"][ptr[i]:ptr[i + 1]].astype(np.int64) for i, kl in enumerate(keys)}
    info = {"pairs": pairs, "distance2": {kl: out["dist2"][ptr[i]:ptr[i + 1]] for i, kl in enumerate(keys)}, "timings_ms": out["timings_ms"]}
    info.update({k: out[k] for k in _mvba.MATCH_COUNTS})
    if return_nn:
        qptr = np.concatenate([[0], np.cumsum(np.diff(kp_ptr)[pairs[:, 0]])])
        for name, key in (("nn_best", "nn_best"), ("nn_distance2", "nn_dist2"), ("nn_second2", "nn_second2")):
            info[name] = {kl: out[key][qptr[i]:qptr[i + 1]] for i, kl in enumerate(keys)}
    return matches, info
