"""NumPy restatement of the two-view entry points (include/mvba.h: mvba_covisibility, mvba_two_view) and of the driver built
on them (lib/initialization.py: relative_pose, bootstrap) -- the definitions written out plainly, with ``np.linalg.eigh`` where
the library runs its Jacobi, and tests/_init_ref.py where the driver triangulates and resects.  Test infrastructure only."""
import numpy as np

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


def relative_pose(pt_ptr, cam_idx, xy, K, pair, n_refine=2, F=None):
    """(R (2, 3, 3), t (2, 3), X (N, 3), info) as lib.initialization.relative_pose; ``F``: use this matrix."""
    k, l = pair
    n, m = len(pt_ptr) - 1, len(K)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ids, xk, xl = shared(pt_ptr, cam_idx, xy, k, l)
    if F is None:
        F, _, st = fundamental(xk, xl)
    else:
        st = 0
    R, t, X = np.full((2, 3, 3), np.nan), np.full((2, 3), np.nan), np.full((n, 3), np.nan)
    info = {"n_front": np.zeros(4, np.int64), "status": int(st), "F": F, "n_shared": len(ids), "quality": np.full((n, 3), np.nan)}
    if st != 0:
        return R, t, X, info
    cands = pose_candidates(K[l].T @ F @ K[k])
    K2, z = np.stack([K[k], K[l]]), np.stack([xk, xl], axis=1)  # the shared points alone, dense: camera 0 = k, 1 = l

    def tri(c, nr):
        R2, t2 = np.stack([np.eye(3), cands[c][0]]), np.stack([np.zeros(3), cands[c][1]])
        Xc, q, s = ref.triangulate(K2, R2, t2, None, None, z, nr)
        return Xc, q, (s == 0) & (q[:, 1] > 0)

    for c in range(4):
        info["n_front"][c] = tri(c, 0)[2].sum()
    best = int(np.argmax(info["n_front"]))
    if not 2 * info["n_front"][best] > len(ids):
        info["status"] = 3
        return R, t, X, info
    Xc, q, front = tri(best, n_refine)
    X[ids[front]], info["quality"][ids[front]] = Xc[front], q[front]
    R[0], t[0] = np.eye(3), 0.0
    R[1], t[1] = cands[best]
    return R, t, X, info


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
    """(R, t, X, info) as lib.initialization.bootstrap, on the host; ``K`` (m, 3, 3) projects to the units of xy."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    m, n = len(K), len(pt_ptr) - 1
    if start_pair is None:
        count = covisibility(pt_ptr, cam_idx, m)
        ks, ls = np.triu_indices(m, 1)
        order = np.argsort(-count[ks, ls], kind="stable")
        tried = [(int(ks[i]), int(ls[i])) for i in order if count[ks[i], ls[i]] >= 8][:16]
    else:
        tried = [tuple(start_pair)]
    best = None
    for pair in tried:
        R2, t2, X2, pi = relative_pose(pt_ptr, cam_idx, xy, K, pair)
        if pi["status"] == 0:
            angle = float(np.nanmedian(pi["quality"][:, 2]))
            if best is None or angle > best[0]:
                best = (angle, pair, R2, t2, X2)
    if best is None:
        raise ValueError("no start pair")
    _, pair, R2, t2, X = best
    R, t = np.full((m, 3, 3), np.nan), np.full((m, 3), np.nan)
    R[list(pair)], t[list(pair)] = R2, t2
    camera_ok = np.zeros(m, bool)
    camera_ok[list(pair)] = True
    point_ok = np.isfinite(X).all(axis=1)
    order = list(pair)
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    seen = np.zeros((n, m), bool)
    seen[pt, cam_idx] = True
    while not camera_ok.all():
        P, _, st = ref.resect(np.where(point_ok[:, None], X, 0.0), pt_ptr, cam_idx, xy, m, point_ok=point_ok)
        usable = np.bincount(cam_idx[point_ok[pt]], minlength=m)
        cand = np.nonzero(~camera_ok & (st == 0) & (usable >= min_points))[0]
        if len(cand) == 0:
            break
        c = int(cand[np.argmax(usable[cand])])
        R[c], t[c] = pose_for_intrinsics(P[c].reshape(3, 4), K[c], X[point_ok & seen[:, c]].mean(axis=0))
        camera_ok[c] = True
        order.append(c)
        ptr, cam, z, _, ids = restrict(pt_ptr, cam_idx, xy, np.ones(n, bool), camera_ok)
        X, q, s = ref.triangulate(K[ids], R[ids], t[ids], ptr, cam, z, 2)
        point_ok = (s == 0) & (q[:, 1] > 0)
        if max_rms is not None:
            point_ok &= q[:, 0] <= max_rms
        X[~point_ok] = np.nan
    for c in (0, 1):
        if not camera_ok[c]:
            raise ValueError(f"camera {c} could not be registered")
    R0, t0, s = R[0].copy(), t[0].copy(), np.linalg.norm(t[1] - t[0])
    X, R, t = ((X - t0) @ R0) / s, R0.T @ R, ((t - t0) @ R0) / s
    axis = "x-right_z-forward" if abs(t[1, 0]) >= abs(t[1, 1]) else "x-up_z-forward"
    return R, t, X, {"axis": axis, "camera_ok": camera_ok, "point_ok": point_ok, "order": order, "start_pair": pair}


def rms_reprojection(K, R, t, X, pt_ptr, cam_idx, xy):
    P = ref.camera_matrices(K, R, t)
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    p = np.einsum("oij,oj->oi", P[cam_idx][:, :, :3], X[pt]) + P[cam_idx][:, :, 3]
    r = p[:, :2] / p[:, 2:3] - xy
    return np.sqrt((r * r).sum(axis=1).mean())
