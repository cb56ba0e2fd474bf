"""NumPy restatement of the initialisation entry points (include/mvba.h: mvba_triangulate, mvba_resect) -- the definitions
written out plainly, with ``np.linalg.eigh`` where the library runs its Jacobi.  Test infrastructure only; the project's own
code (like _covariance_ref.py)."""
import numpy as np

REL_PIVOT = 1e-12


def camera_matrices(K, R, t):
    """P_k = K_k [R_k^T | -R_k^T t_k], (m, 3, 4)."""
    Rt = np.transpose(R, (0, 2, 1))
    return K @ np.concatenate([Rt, -(Rt @ t[:, :, None])], axis=2)


def dense_list(n_points, n_images):
    return (np.arange(0, (n_points + 1) * n_images, n_images, dtype=np.int64),
            np.tile(np.arange(n_images, dtype=np.int32), n_points))


def point_rows(P, cams, xy):
    """The 2 deg unit rows x P[2] - P[0], y P[2] - P[1] of one point, (2 deg, 4), observation by observation."""
    Pk = P[cams]
    rows = np.stack([xy[:, 0, None] * Pk[:, 2] - Pk[:, 0], xy[:, 1, None] * Pk[:, 2] - Pk[:, 1]], axis=1).reshape(-1, 4)
    return rows / np.linalg.norm(rows, axis=1, keepdims=True)


def _project(P, X):
    p = P[:, :, :3] @ X + P[:, :, 3]
    return p[:, :2] / p[:, 2:3], p


def _eval(Pk, xy, X):
    """cost, J^T J, J^T r of sum |pi(P X) - xy|^2 at X."""
    proj, p = _project(Pk, X)
    r = proj - xy
    J = (Pk[:, :2, :3] * p[:, 2, None, None] - p[:, :2, None] * Pk[:, 2, None, :3]) / (p[:, 2] ** 2)[:, None, None]
    return float((r * r).sum()), np.einsum("oij,oik->jk", J, J), np.einsum("oij,oi->j", J, r)


def triangulate_point(P, R, t, cams, xy, n_refine, linear="eigh"):
    """(X, quality, status) of one point; ``linear``: "eigh" of M = rows^T rows (the definition) or "svd" of the rows."""
    nan3 = np.full(3, np.nan)
    if len(cams) < 2:
        return nan3, nan3, 1
    rows = point_rows(P, cams, xy)
    if linear == "eigh":
        w, V = np.linalg.eigh(rows.T @ rows)
        v = V[:, 0]
    else:
        _, s, Vt = np.linalg.svd(rows, full_matrices=True)
        w = np.concatenate([s, np.zeros(4 - len(s))])[::-1] ** 2
        v = Vt[3]
    if not w[1] > REL_PIVOT * w[3]:
        return nan3, nan3, 2
    if not abs(v[3]) > REL_PIVOT:
        return nan3, nan3, 3
    X = v[:3] / v[3]
    Pk = P[cams]
    with np.errstate(all="ignore"):
        E, H, g = _eval(Pk, xy, X)
        for _ in range(n_refine):
            try:
                L = np.linalg.cholesky(H)
            except np.linalg.LinAlgError:
                break
            Xn = X - np.linalg.solve(L.T, np.linalg.solve(L, g))
            En, Hn, gn = _eval(Pk, xy, Xn)
            if not En <= E:
                break
            X, E, H, g = Xn, En, Hn, gn
    if not (np.isfinite(X).all() and np.isfinite(E)):
        return nan3, nan3, 3
    rays = X - t[cams]
    depth = np.einsum("oi,oi->o", R[cams][:, :, 2], rays).min()
    i, j = np.triu_indices(len(cams), 1)
    ang = np.arctan2(np.linalg.norm(np.cross(rays[i], rays[j]), axis=1), (rays[i] * rays[j]).sum(axis=1)).max()
    return X, np.array([np.sqrt(E / len(cams)), depth, ang]), 0


def triangulate(K, R, t, pt_ptr, cam_idx, xy, n_refine=2, n_points=None, linear="eigh"):
    """X (N, 3), quality (N, 3), status (N,) int32.  pt_ptr None: the dense grid, xy (N, m, 2)."""
    K, R, t = (np.asarray(v, np.float64) for v in (K, R, t))
    if pt_ptr is None:
        xy = np.asarray(xy, np.float64)
        pt_ptr, cam_idx = dense_list(xy.shape[0], K.shape[0])
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = len(pt_ptr) - 1
    P = camera_matrices(K, R, t)
    X, q, st = np.empty((n, 3)), np.empty((n, 3)), np.empty(n, np.int32)
    for a in range(n):
        o = slice(pt_ptr[a], pt_ptr[a + 1])
        X[a], q[a], st[a] = triangulate_point(P, R, t, cam_idx[o], xy[o], n_refine, linear)
    return X, q, st


def hartley(pts):
    """(centroid, scale): scale * (pts - centroid) has mean squared distance dim."""
    c = pts.mean(axis=0)
    return c, np.sqrt(pts.shape[1]) / np.sqrt(((pts - c) ** 2).sum(axis=1).mean())


def dlt_rows(Xn, xn):
    """The normalised DLT rows [X~, 0, -x X~], [0, X~, -y X~], (2 n, 12)."""
    h = np.concatenate([Xn, np.ones((len(Xn), 1))], axis=1)
    z = np.zeros_like(h)
    return np.stack([np.concatenate([h, z, -xn[:, 0, None] * h], axis=1),
                     np.concatenate([z, h, -xn[:, 1, None] * h], axis=1)], axis=1).reshape(-1, 12)


def resect_camera(Xk, xk, linear="eigh"):
    """(P (3, 4), quality (2,), status) of one camera from its usable observations."""
    nanP, nan2 = np.full((3, 4), np.nan), np.full(2, np.nan)
    if len(Xk) < 6:
        return nanP, nan2, 1
    with np.errstate(all="ignore"):
        c3, s3 = hartley(Xk)
        c2, s2 = hartley(xk)
        rows = dlt_rows(s3 * (Xk - c3), s2 * (xk - c2))
        if not np.isfinite(rows).all():
            return nanP, nan2, 2
        if linear == "eigh":
            w, V = np.linalg.eigh(rows.T @ rows)
            p = V[:, 0]
        else:
            _, s, Vt = np.linalg.svd(rows, full_matrices=True)
            w, p = s[::-1] ** 2, Vt[11]
    with np.errstate(all="ignore"):
        ratio = w[0] / w[1]
    if not w[1] > REL_PIVOT * w[11]:
        return nanP, np.array([np.nan, ratio]), 2
    T3 = np.eye(4)
    T3[:3, :3] *= s3
    T3[:3, 3] = -s3 * c3
    T2inv = np.array([[1 / s2, 0, c2[0]], [0, 1 / s2, c2[1]], [0, 0, 1]])
    P = T2inv @ p.reshape(3, 4) @ T3
    P = P * (np.sign(np.linalg.det(P[:, :3])) or 1.0) / np.linalg.norm(P[2, :3])
    proj = (Xk @ P[:, :3].T + P[:, 3])
    r = proj[:, :2] / proj[:, 2:3] - xk
    return P, np.array([np.sqrt((r * r).sum() / len(Xk)), ratio]), 0


def resect(X, pt_ptr, cam_idx, xy, n_images, point_ok=None, linear="eigh"):
    """P (m, 12), quality (m, 2), status (m,) int32."""
    X = np.asarray(X, np.float64)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ok = np.isfinite(X).all(axis=1) if point_ok is None else np.asarray(point_ok) != 0
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    P, q, st = np.empty((n_images, 12)), np.empty((n_images, 2)), np.empty(n_images, np.int32)
    for k in range(n_images):
        sel = (cam_idx == k) & ok[pt]
        Pk, q[k], st[k] = resect_camera(X[pt[sel]], xy[sel], linear)
        P[k] = Pk.reshape(12)
    return P, q, st
