"""NumPy restatement of the two-view entry points (include/mvba.h: mvba_covisibility, mvba_two_view) and of the driver built
on them (lib/initialization.py: relative_pose, bootstrap) -- the definitions written out plainly, with ``np.linalg.eigh`` where
the library runs its Jacobi, tests/_init_ref.py where the driver triangulates and resects, and the driver's control flow in
tests/_bootstrap_ref.py.  Test infrastructure only."""
import numpy as np

import _bootstrap_ref as B
import _init_ref as ref

REL_PIVOT = 1e-12
W90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def _list(pt_ptr, cam_idx, xy, n_images):
    if pt_ptr is None:
        xy = np.asarray(xy, np.float64)
        pt_ptr, cam_idx = ref.dense_list(xy.shape[0], n_images)
    return np.asarray(pt_ptr), np.asarray(cam_idx), np.asarray(xy, np.float64).reshape(-1, 2)


def covisibility(pt_ptr, cam_idx, n_images, n_points=None):
    if pt_ptr is None:
        pt_ptr, cam_idx = ref.dense_list(n_points, n_images)
    vis = np.zeros((len(pt_ptr) - 1, n_images), np.int64)
    vis[np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr)), cam_idx] = 1
    return vis.T @ vis


def shared(pt_ptr, cam_idx, xy, k, l):
    """(point ids, x_k, x_l) of the points seen in both k and l, ascending."""
    n = len(pt_ptr) - 1
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    ok, ol = np.full(n, -1), np.full(n, -1)
    ok[pt[cam_idx == k]] = np.nonzero(cam_idx == k)[0]
    ol[pt[cam_idx == l]] = np.nonzero(cam_idx == l)[0]
    ids = np.nonzero((ok >= 0) & (ol >= 0))[0]
    return ids, xy[ok[ids]], xy[ol[ids]]


def hartley_T(c, s):
    return np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])


def sampson_rms(F, xk, xl):
    hk, hl = np.c_[xk, np.ones(len(xk))], np.c_[xl, np.ones(len(xl))]
    Fx, Ftx = hk @ F.T, hl @ F
    r = (hl * Fx).sum(axis=1)
    return np.sqrt((r * r / (Fx[:, 0] ** 2 + Fx[:, 1] ** 2 + Ftx[:, 0] ** 2 + Ftx[:, 1] ** 2)).sum() / len(xk))


def fundamental(xk, xl, linear="eigh"):
    """(F (3, 3), quality (2,), status) from the shared observations; ``linear``: "eigh" of M = rows^T rows (the definition)
    or "svd" of the stacked rows."""
    nanF, nan2 = np.full((3, 3), np.nan), np.full(2, np.nan)
    if len(xk) < 8:
        return nanF, nan2, 1
    with np.errstate(all="ignore"):
        ck, sk = ref.hartley(xk)
        cl, sl = ref.hartley(xl)
        a, b = sk * (xk - ck), sl * (xl - cl)
        one = np.ones(len(a))
        rows = np.stack([b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0], b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1],
                         a[:, 0], a[:, 1], one], axis=1)
        if not np.isfinite(rows).all():
            return nanF, nan2, 2
        if linear == "eigh":
            w, V = np.linalg.eigh(rows.T @ rows)
            f = V[:, 0]
        else:
            _, s, Vt = np.linalg.svd(rows, full_matrices=len(rows) < 9)  # (the full U of 16 641 rows would be 2 GB)
            w, f = np.concatenate([s, np.zeros(9 - len(s))])[::-1] ** 2, Vt[8]
        ratio = w[0] / w[1]
    if not w[1] > REL_PIVOT * w[8]:
        return nanF, nan2, 2
    U, s, Vt = np.linalg.svd(f.reshape(3, 3))
    F = hartley_T(cl, sl).T @ (U @ np.diag([s[0], s[1], 0.0]) @ Vt) @ hartley_T(ck, sk)
    F = F / np.linalg.norm(F)
    if F.flat[np.argmax(np.abs(F))] < 0:
        F = -F
    return F, np.array([sampson_rms(F, xk, xl), ratio]), 0


def two_view(pt_ptr, cam_idx, xy, n_images, pairs, linear="eigh"):
    """F (P, 3, 3), quality (P, 2), n_shared (P,), status (P,)."""
    pt_ptr, cam_idx, xy = _list(pt_ptr, cam_idx, xy, n_images)
    pairs = np.asarray(pairs).reshape(-1, 2)
    F, q = np.empty((len(pairs), 3, 3)), np.empty((len(pairs), 2))
    ns, st = np.empty(len(pairs), np.int64), np.empty(len(pairs), np.int32)
    for i, (k, l) in enumerate(pairs):
        ids, xk, xl = shared(pt_ptr, cam_idx, xy, k, l)
        F[i], q[i], st[i] = fundamental(xk, xl, linear)
        ns[i] = len(ids)
    return F, q, ns, st


def pose_candidates(E):
    """The four (R, t) of the second camera (x_l ~ R^T (X - t), |t| = 1), the first at the origin."""
    U, _, Vt = np.linalg.svd(E)
    U, Vt = U * np.sign(np.linalg.det(U)), Vt * np.sign(np.linalg.det(Vt))
    return [(Rrel.T, -Rrel.T @ tau) for Rrel in (U @ W90 @ Vt, U @ W90.T @ Vt) for tau in (U[:, 2], -U[:, 2])]


def restrict(pt_ptr, cam_idx, xy, point_ok, camera_ok):
    """(pt_ptr, cam_idx, xy, point_ids, camera_ids) of the marked points and cameras, renumbered in ascending order."""
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    pid, cid = np.nonzero(point_ok)[0], np.nonzero(camera_ok)[0]
    keep = [o for o in range(len(cam_idx)) if point_ok[pt[o]] and camera_ok[cam_idx[o]]]
    deg = np.zeros(len(pid), np.int64)
    for o in keep:
        deg[np.searchsorted(pid, pt[o])] += 1
    cam = np.array([np.searchsorted(cid, cam_idx[o]) for o in keep], np.int32)
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), cam, xy[keep], pid, cid


def choose_candidate(K, pair, cands, ids, xk, xl, info, n_refine, by_rms=False, candidate=None):
    """(R (2, 3, 3), t (2, 3), X (N, 3), best): the candidate selection of every relative_pose reference.  ``cands``: four
    (R, t, ...) of camera l = pair[1] with camera k at the origin, each triangulated without refinement over the points ``ids``
    alone (dense: camera 0 = k with ``xk``, 1 = l with ``xl``); info["n_front"] gets the points of status 0 and smallest depth > 0.
    The winner is the first with the most of them; with ``by_rms`` (the homography's rule) the smallest (-n_front, rms, index),
    info["rms"] and info["ambiguous"] -- a second candidate has as many -- are set, and ``candidate`` takes that one instead.  It
    must put more than half of ``ids`` in front -- otherwise info["status"] = 3, best = None and all is NaN -- and is triangulated
    again with ``n_refine`` into X and info["quality"]."""
    k, l = pair
    R, t, X = no_pose(len(info["quality"]))
    K2, z = np.stack([K[k], K[l]]), np.stack([xk, xl], axis=1)

    def tri(c, nr):
        R2, t2 = np.stack([np.eye(3), cands[c][0]]), np.stack([np.zeros(3), cands[c][1]])
        Xc, q, s = ref.triangulate(K2, R2, t2, None, None, z, nr)
        return Xc, q, (s == 0) & (q[:, 1] > 0)

    for c in range(4):
        _, q, front = tri(c, 0)
        info["n_front"][c] = front.sum()
        if by_rms and front.any():
            info["rms"][c] = np.sqrt(np.mean(q[front, 0] ** 2))
    best = int(np.argmax(info["n_front"]))
    if by_rms:
        best = min(range(4), key=lambda c: (-info["n_front"][c], info["rms"][c], c))
        info["ambiguous"] = bool((info["n_front"] >= info["n_front"][best]).sum() > 1)
        if candidate is not None:
            best = candidate
    if not 2 * info["n_front"][best] > len(ids):
        info["status"] = 3
        return R, t, X, None
    Xc, q, front = tri(best, n_refine)
    X[ids[front]], info["quality"][ids[front]] = Xc[front], q[front]
    R[0], t[0] = np.eye(3), 0.0
    R[1], t[1] = cands[best][:2]
    return R, t, X, best


def no_pose(n):
    """(R, t, X) of a relative pose that was not found: NaN."""
    return np.full((2, 3, 3), np.nan), np.full((2, 3), np.nan), np.full((n, 3), np.nan)


def relative_pose(pt_ptr, cam_idx, xy, K, pair, n_refine=2, F=None):
    """(R (2, 3, 3), t (2, 3), X (N, 3), info) as lib.initialization.relative_pose; ``F``: use this matrix."""
    k, l = pair
    n = len(pt_ptr) - 1
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ids, xk, xl = shared(pt_ptr, cam_idx, xy, k, l)
    if F is None:
        F, _, st = fundamental(xk, xl)
    else:
        st = 0
    info = {"n_front": np.zeros(4, np.int64), "status": int(st), "F": F, "n_shared": len(ids), "quality": np.full((n, 3), np.nan)}
    if st != 0:
        return (*no_pose(n), info)
    return (*choose_candidate(K, pair, pose_candidates(K[l].T @ F @ K[k]), ids, xk, xl, info, n_refine)[:3], info)


def pose_for_intrinsics(P, K, c):
    """(R, t) of a camera with the GIVEN intrinsics K that images the neighbourhood of the point c as P does: the rotation of
    P's RQ decomposition (positive diagonal), and the centre moved along the ray of c so that c keeps its image and its
    magnification f / depth.  (P's own centre belongs to P's own focal length: the DLT trades the two against each other.)"""
    M = P[:, :3] * np.sign(np.linalg.det(P[:, :3]))
    flip = np.eye(3)[::-1]
    q, r = np.linalg.qr((flip @ M).T)
    Ku, Rc = flip @ r.T @ flip, flip @ q.T
    s = np.sign(np.diag(Ku))
    Ku, R = Ku * s, (s[:, None] * Rc).T
    Ku = Ku / Ku[2, 2]
    y = R.T @ (c + np.linalg.solve(P[:, :3], P[:, 3]))  # c in P's camera frame
    f = 0.5 * (Ku[0, 0] + Ku[1, 1])  # (decompose_projection's model: one focal length, the skew dropped)
    x = f * y[:2] / y[2] + Ku[:2, 2]  # its image
    d = y[2] * K[0, 0] / f
    return R, c - R @ (d * np.array([(x[0] - K[0, 2]) / K[0, 0], (x[1] - K[1, 2]) / K[1, 1], 1.0]))


def bootstrap(pt_ptr, cam_idx, xy, K, start_pair=None, min_points=12, max_rms=None):
    """(R, t, X, info) as lib.initialization.bootstrap without a threshold, on the host: the driver of tests/_bootstrap_ref.py with
    the plain form of each step; ``K`` (m, 3, 3) projects to the units of xy."""
    R, t, X, info, _ = B.bootstrap(pt_ptr, cam_idx, xy, K, lambda pair: relative_pose(pt_ptr, cam_idx, xy, K, pair),
                                   register_plain(pt_ptr, cam_idx, xy, K, min_points), triangulate_plain, start_pair, max_rms)
    return R, t, X, {key: info[key] for key in B.PLAIN_KEYS}


def register_plain(pt_ptr, cam_idx, xy, K, min_points):
    """The registration step of tests/_bootstrap_ref.py in its plain form: every camera resected from the current points; the
    unregistered one of status 0 with the most usable observations (at least ``min_points``, the lowest index on ties) is taken,
    its pose from ``pose_for_intrinsics`` at the centroid of the points it sees.  It verifies nothing: ``dropped`` is None."""
    pt_ptr, cam_idx, xy = np.asarray(pt_ptr), np.asarray(cam_idx), np.asarray(xy, np.float64).reshape(-1, 2)
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))

    def register(X, point_ok, camera_ok):
        P, _, st = ref.resect(np.where(point_ok[:, None], X, 0.0), pt_ptr, cam_idx, xy, len(K), point_ok=point_ok)
        usable = np.bincount(cam_idx[point_ok[pt]], minlength=len(K))
        cand = np.nonzero(~camera_ok & (st == 0) & (usable >= min_points))[0]
        if len(cand) == 0:
            return None
        c = int(cand[np.argmax(usable[cand])])
        sel = point_ok[pt] & (cam_idx == c)
        return (c, *pose_for_intrinsics(P[c].reshape(3, 4), K[c], X[pt[sel]].mean(axis=0)), sel, None)

    return register


def triangulate_plain(K, R, t, ptr, cam, xy):
    """The triangulation step of tests/_bootstrap_ref.py in its plain form: every observation of the list is used."""
    X, q, s = ref.triangulate(K, R, t, ptr, cam, xy, 2)
    return X, q, s, np.ones(len(cam), bool), {}


def rms_reprojection(K, R, t, X, pt_ptr, cam_idx, xy):
    P = ref.camera_matrices(K, R, t)
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    p = np.einsum("oij,oj->oi", P[cam_idx][:, :, :3], X[pt]) + P[cam_idx][:, :, 3]
    r = p[:, :2] / p[:, 2:3] - xy
    return np.sqrt((r * r).sum(axis=1).mean())
