"""NumPy restatement of the robust resection entry point (include/mvba.h: mvba_resect_robust, mvba_resect_sample) and of the
driver that uses it (lib/initialization.py: bootstrap with ``resect_threshold``) -- the definitions written out plainly on
tests/_init_ref.py (hartley, dlt_rows, resect_camera) and tests/_ransac_ref.py (mix), with ``np.linalg.eigh`` of the moment
matrix (or the SVD of the stacked rows) where the device runs its own Jacobi.  Test infrastructure only."""
import numpy as np

import _bootstrap_ref as B
import _init_ref as ref
import _ransac_ref as RR
import _twoview_ref as T

MIN_OBS = 6


def sample(seed, k, h, n):
    """The 6 distinct indices below n of hypothesis h of camera k: _ransac_ref.sample's generator with l = k, 6 draws."""
    s = RR.mix(RR.mix(RR.mix(seed & RR.MASK) ^ ((k << 32) | k)) ^ h)
    idx = []
    while len(idx) < 6:
        s = RR.mix(s)
        j = ((s >> 32) * n) >> 32
        if j not in idx:
            idx.append(j)
    return np.array(idx, np.int64)


def reprojection(P, Xk, xk):
    """(squared reprojection distances, depths), each (..., n), of the observations under P (..., 3, 4)."""
    with np.errstate(all="ignore"):
        p = np.einsum("...ij,nj->...ni", P[..., :3], Xk) + P[..., None, :, 3]
        r = p[..., :2] / p[..., 2:3] - xk
        return (r * r).sum(axis=-1), p[..., 2]


def _setup(Xk, xk):
    """(T2^-1, T3, normalised DLT rows (n, 2, 12)) of a camera's usable observations."""
    c3, s3 = ref.hartley(Xk)
    c2, s2 = ref.hartley(xk)
    T3 = np.eye(4)
    T3[:3, :3] *= s3
    T3[:3, 3] = -s3 * c3
    T2inv = np.array([[1 / s2, 0, c2[0]], [0, 1 / s2, c2[1]], [0, 0, 1]])
    return T2inv, T3, ref.dlt_rows(s3 * (Xk - c3), s2 * (xk - c2)).reshape(-1, 2, 12)


def _hypotheses(rows, T2inv, T3, k, seed, hs, linear):
    """The hypotheses ``hs`` of camera k: P (len(hs), 3, 4), NaN where degenerate, and the pivots lambda_2 / lambda_max."""
    n = len(rows)
    r12 = np.stack([rows[sample(seed, k, int(h), n)].reshape(12, 12) for h in hs])
    Ph, pivot = np.full((len(hs), 3, 4), np.nan), np.full(len(hs), np.nan)
    fin = np.isfinite(r12).all(axis=(1, 2))
    if not fin.any():
        return Ph, pivot
    r = r12[fin]
    if linear == "eigh":
        w, V = np.linalg.eigh(np.transpose(r, (0, 2, 1)) @ r)
        p = V[:, :, 0]
    else:
        _, s, Vt = np.linalg.svd(r, full_matrices=True)
        w, p = s[:, ::-1] ** 2, Vt[:, 11]
    pivot[fin] = w[:, 1] / w[:, 11]
    P = T2inv @ p.reshape(-1, 3, 4) @ T3
    sign = np.where(np.linalg.det(P[:, :, :3]) < 0, -1.0, 1.0)
    P = P * (sign / np.linalg.norm(P[:, 2, :3], axis=1))[:, None, None]
    good = (w[:, 1] > ref.REL_PIVOT * w[:, 11]) & np.isfinite(P).all(axis=(1, 2))
    Ph[np.nonzero(fin)[0][good]] = P[good]
    return Ph, pivot


def _score(Ph, Xk, xk, thr2):
    """(counts (H,), inlier (H, n), d2 (H, n), margin) of the hypotheses Ph."""
    ok = np.isfinite(Ph).all(axis=(1, 2))
    d2, depth = reprojection(Ph, Xk, xk)
    with np.errstate(all="ignore"):
        inl = (depth > 0) & (d2 <= thr2)
        margin = np.nanmin(np.abs(d2[ok] / thr2 - 1.0)) if ok.any() else np.inf
    return np.where(ok, inl.sum(axis=1), -1).astype(np.int32), inl, d2, margin


def hypothesis_counts(Xk, xk, k, threshold, seed, hs, linear="eigh"):
    """(counts, margin, pivot) of the entries ``hs`` of the camera's count table alone (a hypothesis depends on (seed, k, h) only)."""
    if len(Xk) < MIN_OBS:
        return np.full(len(hs), -1, np.int32), np.inf, np.full(len(hs), np.nan)
    with np.errstate(all="ignore"):
        T2inv, T3, rows = _setup(Xk, xk)
        Ph, pivot = _hypotheses(rows, T2inv, T3, k, seed, hs, linear)
    counts, _, _, margin = _score(Ph, Xk, xk, threshold * threshold)
    return counts, margin, pivot


def robust_resect_camera(Xk, xk, k, threshold, n_hyp, seed, n_refit, linear="eigh"):
    """One camera from its usable observations in ascending point order.  A dict: P (3, 4), quality (2,), status, n_inliers,
    best, mask (n,), hyp_count (H,), the figures of the parity premises: ``margin`` -- the smallest |d^2 / threshold^2 - 1| over
    every distance compared with the threshold -- and ``pivot`` (H,) -- lambda_2 / lambda_max of each hypothesis --, and the
    trace of the refit loop: ``n_accepted``, ``n_changed`` (kept refits whose inlier set differs from the one before), ``sizes``
    (the inlier counts |I_0|, |I_1|, ... of P_best and of every refit that was evaluated, -1 padded to 1 + n_refit) and ``end``
    -- "rejected", "solver", "exhausted", or "" for a camera whose status is not 0."""
    n, H, thr2 = len(Xk), int(n_hyp), threshold * threshold
    out = {"P": np.full((3, 4), np.nan), "quality": np.full(2, np.nan), "status": 1, "n_inliers": 0, "best": -1,
           "mask": np.zeros(n, bool), "hyp_count": np.full(H, -1, np.int32), "margin": np.inf, "pivot": np.full(H, np.nan),
           "n_accepted": 0, "n_changed": 0, "sizes": np.full(1 + n_refit, -1), "end": ""}
    if n < MIN_OBS:
        return out
    with np.errstate(all="ignore"):
        T2inv, T3, rows = _setup(Xk, xk)
        Ph, out["pivot"] = _hypotheses(rows, T2inv, T3, k, seed, range(H), linear)
    out["hyp_count"], inl, d2, out["margin"] = _score(Ph, Xk, xk, thr2)
    best = int(np.argmax(out["hyp_count"]))
    if out["hyp_count"][best] < 0:
        out["status"] = 2
        return out
    out["best"] = best
    if out["hyp_count"][best] < MIN_OBS:
        out["status"] = 4
        return out
    mask, dd = inl[best], d2[best]
    P, ratio, end, n_acc, n_chg = Ph[best], 0.0, "exhausted", 0, 0
    out["sizes"][0] = mask.sum()
    for r in range(1, n_refit + 1):
        Pr, q, st = ref.resect_camera(Xk[mask], xk[mask], linear)
        if st != 0:
            end = "solver"
            break
        dr, depth = reprojection(Pr, Xk, xk)
        out["margin"] = min(out["margin"], np.abs(dr / thr2 - 1.0).min())
        new = (depth > 0) & (dr <= thr2)
        out["sizes"][r] = new.sum()
        if new.sum() < (MIN_OBS if r == 1 else mask.sum()):
            end = "rejected"
            break
        n_acc, n_chg = n_acc + 1, n_chg + int(not np.array_equal(new, mask))
        P, ratio, mask, dd = Pr, q[1], new, dr
    out.update(P=P, quality=np.array([np.sqrt(dd[mask].sum() / mask.sum()), ratio]), status=0, n_inliers=int(mask.sum()), mask=mask,
               n_accepted=n_acc, n_changed=n_chg, end=end)
    return out


def resect_robust(X, pt_ptr, cam_idx, xy, n_images, threshold, point_ok=None, cameras=None, n_hyp=512, seed=0, n_refit=2, linear="eigh"):
    """A dict of arrays over the listed cameras: P (C, 3, 4), quality (C, 2), n_usable, n_inliers, best, status (C,), hyp_count
    (C, H), inlier (n_obs,), margin (C,), pivot (C, H) and the refit trace n_accepted, n_changed, sizes, end.  pt_ptr None: the
    dense grid, xy (N, m, 2)."""
    X = np.asarray(X, np.float64)
    if pt_ptr is None:
        pt_ptr, cam_idx = ref.dense_list(len(X), n_images)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ok = np.isfinite(X).all(axis=1) if point_ok is None else np.asarray(point_ok) != 0
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    cameras = np.arange(n_images) if cameras is None else np.asarray(cameras)
    inlier, res, nu = np.zeros(len(xy), bool), [], []
    for k in cameras:
        obs = np.nonzero((cam_idx == k) & ok[pt])[0]
        r = robust_resect_camera(X[pt[obs]], xy[obs], int(k), threshold, n_hyp, seed, n_refit, linear)
        inlier[obs[r["mask"]]] = True
        res.append(r)
        nu.append(len(obs))
    out = {key: np.array([r[key] for r in res]) for key in ("P", "quality", "n_inliers", "best", "status", "hyp_count", "margin", "pivot",
                                                            "n_accepted", "n_changed", "sizes", "end")}
    out.update(n_usable=np.array(nu, np.int64), inlier=inlier)
    for v in out.values():
        v.setflags(write=False)
    return out


def bootstrap(pt_ptr, cam_idx, xy, K, resect_threshold, n_hyp=512, seed=0, start_pair=None, min_points=12, max_rms=None, linear="eigh"):
    """(R, t, X, info) as lib.initialization.bootstrap with ``resect_threshold`` (and no ``ransac_threshold``), on the host: the
    driver of tests/_bootstrap_ref.py with the robust resection below as its registration step, and tests/_twoview_ref.py's plain
    relative_pose and triangulation.  ``K`` (m, 3, 3) projects to the units of xy."""
    R, t, X, info, _ = B.bootstrap(pt_ptr, cam_idx, xy, K, lambda pair: T.relative_pose(pt_ptr, cam_idx, xy, K, pair),
                                   register_robust(pt_ptr, cam_idx, xy, K, resect_threshold, min_points, n_hyp, seed, linear), T.triangulate_plain,
                                   start_pair, max_rms)
    return R, t, X, {key: info[key] for key in B.ROBUST_KEYS}


def register_robust(pt_ptr, cam_idx, xy, K, threshold, min_points, n_hyp=512, seed=0, linear="eigh"):
    """The registration step of tests/_bootstrap_ref.py with ``resect_threshold``: the robust resection of the unregistered
    cameras, ``most_inliers`` of them, the pose from ``pose_for_intrinsics`` at the centroid of its inlier points."""
    pt_ptr, cam_idx, xy = np.asarray(pt_ptr), np.asarray(cam_idx), np.asarray(xy, np.float64).reshape(-1, 2)
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))

    def register(X, point_ok, camera_ok):
        todo = np.nonzero(~camera_ok)[0]
        ri = resect_robust(np.where(point_ok[:, None], X, 0.0), pt_ptr, cam_idx, xy, len(K), threshold, point_ok=point_ok, cameras=todo,
                           n_hyp=n_hyp, seed=seed, n_refit=2, linear=linear)
        pick = B.most_inliers(ri, todo, cam_idx, point_ok[pt], min_points)
        if pick is None:
            return None
        i, c, sel, dropped = pick
        return (c, *T.pose_for_intrinsics(ri["P"][i], K[c], X[pt[sel]].mean(axis=0)), sel, dropped)

    return register
