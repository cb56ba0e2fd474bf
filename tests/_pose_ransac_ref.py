"""NumPy restatement of the calibrated robust resection (include/mvba.h: mvba_pose_robust, mvba_pose_refine, mvba_pose_sample)
and of the driver that uses it (lib/initialization.py: bootstrap with ``pose_threshold``) -- the header comment written out
plainly, with two routes where the device has one: the quartic's roots by ``np.roots`` ("roots") or by the Ferrari
factorisation the header describes ("ferrari": an independent finder), and the Gauss-Newton step by the Cholesky factor of the
6 x 6 normal matrix ("chol") or by ``lstsq`` on the stacked rows ("lstsq").  Test infrastructure only."""
import numpy as np

import _bootstrap_ref as B
import _init_ref as ref
import _ransac_ref as RR
import _resect_ransac_ref as QR
import _twoview_ref as T

MIN_OBS, MIN_REFINE_OBS = 4, 3
ROOT_ITERS = 50
IMAG_TOL = 1e-8  # a root of np.roots is real if |imag| <= this x max(1, |root|)


def sample(seed, k, h, n):
    """The 4 distinct indices below n of hypothesis h of camera k: _ransac_ref.sample's generator with l = k, 4 draws."""
    s = RR.mix(RR.mix(RR.mix(seed & RR.MASK) ^ ((k << 32) | k)) ^ h)
    idx = []
    while len(idx) < 4:
        s = RR.mix(s)
        j = ((s >> 32) * n) >> 32
        if j not in idx:
            idx.append(j)
    return np.array(idx, np.int64)


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    n = w / th
    nx = np.array([[0.0, -n[2], n[1]], [n[2], 0.0, -n[0]], [-n[1], n[0], 0.0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * nx + (1.0 - np.cos(th)) * np.outer(n, n)


def camera_matrix(K, R, t):
    """K [R^T | -R^T t], (..., 3, 4)."""
    Rt = np.swapaxes(R, -1, -2)
    return K @ np.concatenate([Rt, -(Rt @ t[..., None])], axis=-1)


def bearings(K, z):
    """K^-1 (x, y, 1) scaled to unit length, (..., 3)."""
    v = np.linalg.solve(K, np.concatenate([z, np.ones(z.shape[:-1] + (1,))], axis=-1)[..., None])[..., 0]
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _frame(A0, A1, A2):
    """(F (..., 3, 3) with e1, e2, e3 in its columns, ok): the Gram-Schmidt frame of the triangles."""
    e1 = A1 - A0
    w = A2 - A0
    e1 = e1 / np.linalg.norm(e1, axis=-1, keepdims=True)
    rem = w - (e1 * w).sum(axis=-1, keepdims=True) * e1
    nr = (rem * rem).sum(axis=-1)
    ok = nr > ref.REL_PIVOT * (w * w).sum(axis=-1)
    e2 = rem / np.sqrt(nr)[..., None]
    return np.stack([e1, e2, np.cross(e1, e2)], axis=-1), ok


def _pmul(a, b):
    """Row-wise polynomial product, highest power first."""
    out = np.zeros((len(a), a.shape[1] + b.shape[1] - 1))
    for i in range(a.shape[1]):
        for j in range(b.shape[1]):
            out[:, i + j] += a[:, i] * b[:, j]
    return out


def _quartic(a2, b2, c2, ca, cb, cg):
    """(coefficients (H, 5), highest first; N (H, 3); D (H, 2)) of the quartic in v = s2 / s0: u = N / D from the difference of
    the first and third equations, then D^2 (1 - r W) + N^2 - 2 cos gamma N D = 0 from the third."""
    q, r = (a2 - c2) / b2, c2 / b2
    one, zero = np.ones_like(q), np.zeros_like(q)
    N = np.stack([q - 1.0, -2.0 * q * cb, q + 1.0], axis=1)
    D = np.stack([-2.0 * ca, 2.0 * cg], axis=1)
    W = np.stack([one, -2.0 * cb, one], axis=1)
    rW = np.stack([zero, zero, one], axis=1) - r[:, None] * W
    ND = _pmul(N, D)
    out = _pmul(_pmul(D, D), rW) + _pmul(N, N)
    out[:, 1:] -= 2.0 * cg[:, None] * ND
    return out, N, D


def _roots_numpy(A):
    """The real roots of each quartic by np.roots, (H, 4), NaN where there is none."""
    v = np.full((len(A), 4), np.nan)
    for i, a in enumerate(A):
        if not np.isfinite(a).all() or a[0] == 0.0:
            continue
        z = np.roots(a)
        re = z.real[np.abs(z.imag) <= IMAG_TOL * np.maximum(1.0, np.abs(z))]
        v[i, : len(re)] = re
    return v


def _roots_ferrari(A):
    """The same by the factorisation into two quadratics the header describes, (H, 4), NaN where a discriminant is negative."""
    B3, B2, B1, B0 = (A[:, i] / A[:, 0] for i in (1, 2, 3, 4))
    p = B2 - 0.375 * B3 ** 2
    g = B1 - 0.5 * B3 * B2 + 0.125 * B3 ** 3
    h = B0 - 0.25 * B3 * B1 + 0.0625 * B3 ** 2 * B2 - (3.0 / 256.0) * B3 ** 4
    k2, k1, k0 = p, 0.25 * p * p - h, -0.125 * g * g
    hi = 1.0 + np.maximum(np.abs(k2), np.maximum(np.abs(k1), np.abs(k0)))  # the cubic is <= 0 at 0 and > 0 here
    lo, m = np.zeros_like(hi), hi.copy()
    for _ in range(ROOT_ITERS):  # Newton where it stays inside the bracket, bisection where it does not
        fv, fd = ((m + k2) * m + k1) * m + k0, (3.0 * m + 2.0 * k2) * m + k1
        hi, lo = np.where(fv > 0.0, m, hi), np.where(fv > 0.0, lo, m)
        mn = m - fv / fd
        m = np.where((mn > lo) & (mn < hi), mn, 0.5 * (lo + hi))
    s = np.sqrt(2.0 * m)
    gs = g / (2.0 * s)
    q1, q2 = 0.5 * p + m - gs, 0.5 * p + m + gs
    D1, D2 = s * s - 4.0 * q1, s * s - 4.0 * q2
    r1, r2 = np.sqrt(np.where(D1 >= 0, D1, np.nan)), np.sqrt(np.where(D2 >= 0, D2, np.nan))
    y = np.stack([0.5 * (-s - r1), 0.5 * (-s + r1), 0.5 * (s - r2), 0.5 * (s + r2)], axis=1)
    return y - 0.25 * B3[:, None]


def hypotheses(K, Xs, zs, roots="roots"):
    """The poses of H samples: Xs (H, 4, 3), zs (H, 4, 2) -> R (H, 3, 3), t (H, 3), P (H, 3, 4), NaN where degenerate, and
    n_sol (H,), the number of solutions that survived the polish."""
    H = len(Xs)
    with np.errstate(all="ignore"):
        d = bearings(K, zs[:, :3])  # (H, 3, 3)
        a2 = ((Xs[:, 1] - Xs[:, 2]) ** 2).sum(axis=1)
        b2 = ((Xs[:, 0] - Xs[:, 2]) ** 2).sum(axis=1)
        c2 = ((Xs[:, 0] - Xs[:, 1]) ** 2).sum(axis=1)
        ca, cb, cg = (d[:, 1] * d[:, 2]).sum(axis=1), (d[:, 0] * d[:, 2]).sum(axis=1), (d[:, 0] * d[:, 1]).sum(axis=1)
        A, N, D = _quartic(a2, b2, c2, ca, cb, cg)
        v = _roots_numpy(A) if roots == "roots" else _roots_ferrari(A)
        B = A[:, 1:] / A[:, :1]
        for _ in range(2):  # polish on the monic quartic
            fv = (((v + B[:, 0:1]) * v + B[:, 1:2]) * v + B[:, 2:3]) * v + B[:, 3:4]
            fd = ((4.0 * v + 3.0 * B[:, 0:1]) * v + 2.0 * B[:, 1:2]) * v + B[:, 2:3]
            vn = v - fv / fd
            v = np.where(np.isfinite(vn), vn, v)
        col = lambda x: x[:, None]  # noqa: E731
        W = 1.0 + v * v - 2.0 * v * col(cb)
        u = ((col(N[:, 0]) * v + col(N[:, 1])) * v + col(N[:, 2])) / (col(D[:, 0]) * v + col(D[:, 1]))
        s0 = np.sqrt(col(b2) / W)
        s1, s2 = u * s0, v * s0
        FX, okX = _frame(Xs[:, 0], Xs[:, 1], Xs[:, 2])
        ok = col(okX) & (s0 > 0) & (s1 > 0) & (s2 > 0)
        for _ in range(3):  # Newton on the three equations
            F = np.stack([s1 * s1 + s2 * s2 - 2 * s1 * s2 * col(ca) - col(a2), s0 * s0 + s2 * s2 - 2 * s0 * s2 * col(cb) - col(b2),
                          s0 * s0 + s1 * s1 - 2 * s0 * s1 * col(cg) - col(c2)], axis=-1)
            J = np.zeros(v.shape + (3, 3))
            J[..., 0, 1], J[..., 0, 2] = 2 * (s1 - s2 * col(ca)), 2 * (s2 - s1 * col(ca))
            J[..., 1, 0], J[..., 1, 2] = 2 * (s0 - s2 * col(cb)), 2 * (s2 - s0 * col(cb))
            J[..., 2, 0], J[..., 2, 1] = 2 * (s0 - s1 * col(cg)), 2 * (s1 - s0 * col(cg))
            good = np.isfinite(J).all(axis=(-1, -2)) & np.isfinite(F).all(axis=-1) & (np.abs(np.linalg.det(np.where(np.isfinite(J), J, 0.0))) > 0)
            dx = np.full(F.shape, np.nan)
            dx[good] = np.linalg.solve(J[good], F[good][..., None])[..., 0]
            s0, s1, s2 = s0 - dx[..., 0], s1 - dx[..., 1], s2 - dx[..., 2]
        ok &= (s0 > 0) & (s1 > 0) & (s2 > 0) & np.isfinite(s0) & np.isfinite(s1) & np.isfinite(s2)
        Y = np.stack([s0, s1, s2], axis=-1)[..., None] * d[:, None]  # (H, 4, 3 points, 3)
        FY, okY = _frame(Y[:, :, 0], Y[:, :, 1], Y[:, :, 2])
        ok &= okY
        Rcw = FY @ np.swapaxes(FX, -1, -2)[:, None]
        R = np.swapaxes(Rcw, -1, -2)
        t = Xs[:, None, 0] - (R @ Y[:, :, 0, :, None])[..., 0]
        P = camera_matrix(K, R, t)
        p = (P[..., :3] @ Xs[:, None, 3, :, None])[..., 0] + P[..., 3]
        r = p[..., :2] / p[..., 2:3] - zs[:, None, 3]
        d2 = (r * r).sum(axis=-1)
        ok &= (p[..., 2] > 0) & np.isfinite(d2) & np.isfinite(P).all(axis=(-1, -2)) & np.isfinite(R).all(axis=(-1, -2)) & np.isfinite(t).all(axis=-1)
    Ro, to, Po = np.full((H, 3, 3), np.nan), np.full((H, 3), np.nan), np.full((H, 3, 4), np.nan)
    for i in range(H):
        c = np.nonzero(ok[i])[0]
        if len(c):
            j = c[np.lexsort((s0[i, c], d2[i, c]))[0]]  # the smallest distance, the smaller s0 on a tie
            Ro[i], to[i], Po[i] = R[i, j], t[i, j], P[i, j]
    return Ro, to, Po, ok.sum(axis=1)


def pass_sums(K, R, t, Xk, xk):
    """(cost, J (n, 2, 6), e (n, 2)) of the observations at the pose: e = pi(K R^T (X - t)) - xy, J = de / d(delta t, omega)."""
    d = Xk - t
    y = d @ R
    p = y @ K.T
    pi = p[:, :2] / p[:, 2:3]
    e = pi - xk
    Jy = (K[None, :2, :] - pi[:, :, None] * K[None, 2:3, :]) / p[:, 2, None, None]
    A = Jy @ R.T
    J = np.concatenate([-A, np.cross(A, d[:, None, :])], axis=2)
    return float((e * e).sum()), J, e


def gauss_newton(K, R, t, Xk, xk, n_steps, solver="chol"):
    """The iteration of k_pose_step: (R, t, record) with record = cost0, cost, steps, pivot, fail (the step whose normal matrix
    failed the pivot rule, -1: none; 0 also for an input that is not finite) and fail_pivot (the smallest relative pivot of
    that matrix; -1 where the factorisation met a pivot that is not positive)."""
    rec = {"cost0": np.nan, "cost": np.nan, "steps": 0, "pivot": 0.0, "fail": -1, "fail_pivot": np.nan}
    with np.errstate(all="ignore"):
        cost, J, e = pass_sums(K, R, t, Xk, xk)
        rec["cost0"] = rec["cost"] = cost
        if not (np.isfinite(cost) and np.isfinite(R).all() and np.isfinite(t).all()):
            rec["fail"] = 0
            return R, t, rec
        for j in range(n_steps):
            Hm = np.einsum("nri,nrj->ij", J, J)
            g = np.einsum("nri,nr->i", J, e)
            dmax = np.diag(Hm).max()
            try:
                L = np.linalg.cholesky(Hm)
                piv = np.diag(L) ** 2
            except np.linalg.LinAlgError:
                piv = np.array([-1.0])
            if not (piv > ref.REL_PIVOT * dmax).all():
                rec["fail"], rec["fail_pivot"] = j, float((piv / dmax).min())
                break
            rec["pivot"] = float((piv / dmax).min())
            if solver == "chol":
                delta = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            else:
                delta = np.linalg.lstsq(J.reshape(-1, 6), -e.reshape(-1), rcond=None)[0]
            Rn, tn = rodrigues(delta[3:]) @ R, t + delta[:3]
            cn, Jn, en = pass_sums(K, Rn, tn, Xk, xk)
            if not cn <= cost:
                break
            R, t, cost, J, e = Rn, tn, cn, Jn, en
            rec["steps"] += 1
            rec["cost"] = cost
    return R, t, rec


def robust_pose_camera(Xk, xk, K, k, threshold, n_hyp, seed, n_refine, n_refit, roots="roots", solver="chol"):
    """One camera from its usable observations in ascending point order.  A dict: R, t, quality (2,), status, n_inliers, best,
    mask (n,), hyp_count (H,), ``margin`` -- the smallest |d^2 / threshold^2 - 1| over every distance compared with the
    threshold --, ``n_sol`` (H,) and the trace of the refit loop as in _resect_ransac_ref.robust_resect_camera."""
    n, H, thr2 = len(Xk), int(n_hyp), threshold * threshold
    out = {"R": np.full((3, 3), np.nan), "t": np.full(3, np.nan), "quality": np.full(2, np.nan), "status": 1, "n_inliers": 0, "best": -1,
           "mask": np.zeros(n, bool), "hyp_count": np.full(H, -1, np.int32), "margin": np.inf, "n_sol": np.zeros(H, np.int64),
           "n_accepted": 0, "n_changed": 0, "sizes": np.full(1 + n_refit, -1), "end": ""}
    if n < MIN_OBS:
        return out
    idx = np.stack([sample(seed, k, h, n) for h in range(H)])
    Rh, th, Ph, out["n_sol"] = hypotheses(K, Xk[idx], xk[idx], roots)
    out["hyp_count"], inl, d2, out["margin"] = QR._score(Ph, Xk, xk, thr2)
    best = int(np.argmax(out["hyp_count"]))
    if out["hyp_count"][best] < 0:
        out["status"] = 2
        return out
    out["best"] = best
    if out["hyp_count"][best] < MIN_OBS:
        out["status"] = 4
        return out
    mask, dd = inl[best], d2[best]
    R, t, pivot, end, n_acc, n_chg = Rh[best], th[best], 0.0, "exhausted", 0, 0
    out["sizes"][0] = mask.sum()
    for r in range(1, n_refit + 1):
        Rr, tr, rec = gauss_newton(K, R, t, Xk[mask], xk[mask], n_refine, solver)
        if rec["fail"] >= 0:
            end = "solver"
            break
        dr, depth = QR.reprojection(camera_matrix(K, Rr, tr), Xk, xk)
        out["margin"] = min(out["margin"], np.abs(dr / thr2 - 1.0).min())
        new = (depth > 0) & (dr <= thr2)
        out["sizes"][r] = new.sum()
        if new.sum() < mask.sum():
            end = "rejected"
            break
        n_acc, n_chg = n_acc + 1, n_chg + int(not np.array_equal(new, mask))
        R, t, mask, dd = Rr, tr, new, dr
        if n_refine > 0:
            pivot = rec["pivot"]
    out.update(R=R, t=t, quality=np.array([np.sqrt(dd[mask].sum() / mask.sum()), pivot]), status=0, n_inliers=int(mask.sum()), mask=mask,
               n_accepted=n_acc, n_changed=n_chg, end=end)
    return out


def _usable(X, pt_ptr, cam_idx, xy, n_images, point_ok):
    X = np.asarray(X, np.float64)
    if pt_ptr is None:
        pt_ptr, cam_idx = ref.dense_list(len(X), n_images)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ok = np.isfinite(X).all(axis=1) if point_ok is None else np.asarray(point_ok) != 0
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    return X, np.asarray(cam_idx), xy, ok, pt


def pose_robust(X, pt_ptr, cam_idx, xy, K, threshold, point_ok=None, cameras=None, n_hyp=512, seed=0, n_refine=5, n_refit=2, roots="roots",
                solver="chol"):
    """A dict of arrays over the listed cameras: R (C, 3, 3), t (C, 3), quality (C, 2), n_usable, n_inliers, best, status (C,),
    hyp_count (C, H), inlier (n_obs,), margin (C,), n_sol (C, H) and the refit trace.  pt_ptr None: the dense grid."""
    K = np.asarray(K, np.float64)
    m = len(K)
    X, cam_idx, xy, ok, pt = _usable(X, pt_ptr, cam_idx, xy, m, point_ok)
    cameras = np.arange(m) if cameras is None else np.asarray(cameras)
    inlier, res, nu = np.zeros(len(xy), bool), [], []
    for k in cameras:
        obs = np.nonzero((cam_idx == k) & ok[pt])[0]
        r = robust_pose_camera(X[pt[obs]], xy[obs], K[k], int(k), threshold, n_hyp, seed, n_refine, n_refit, roots, solver)
        inlier[obs[r["mask"]]] = True
        res.append(r)
        nu.append(len(obs))
    out = {key: np.array([r[key] for r in res]) for key in ("R", "t", "quality", "n_inliers", "best", "status", "hyp_count", "margin", "n_sol",
                                                            "n_accepted", "n_changed", "sizes", "end")}
    out.update(n_usable=np.array(nu, np.int64), inlier=inlier)
    for v in out.values():
        v.setflags(write=False)
    return out


def pose_refine(X, pt_ptr, cam_idx, xy, K, R, t, point_ok=None, obs_ok=None, cameras=None, n_steps=10, solver="chol", trace=False):
    """(R, t, quality (C, 3), n_usable, status) of mvba_pose_refine; with ``trace`` also the list of gauss_newton's records
    (None for a camera of status 1)."""
    K = np.asarray(K, np.float64)
    m = len(K)
    X, cam_idx, xy, ok, pt = _usable(X, pt_ptr, cam_idx, xy, m, point_ok)
    use = ok[pt] if obs_ok is None else ok[pt] & (np.asarray(obs_ok).reshape(-1) != 0)
    cameras = np.arange(m) if cameras is None else np.asarray(cameras)
    R, t = np.array(R, np.float64).reshape(-1, 3, 3), np.array(t, np.float64).reshape(-1, 3)
    q, nu, st = np.full((len(cameras), 3), np.nan), np.zeros(len(cameras), np.int64), np.ones(len(cameras), np.int32)
    recs = [None] * len(cameras)
    for c, k in enumerate(cameras):
        obs = np.nonzero((cam_idx == k) & use)[0]
        nu[c] = len(obs)
        if len(obs) < MIN_REFINE_OBS:
            continue
        Rn, tn, rec = gauss_newton(K[k], R[c], t[c], X[pt[obs]], xy[obs], n_steps, solver)
        recs[c] = rec
        st[c] = 2 if rec["fail"] == 0 else 0
        if st[c] == 0:
            R[c], t[c] = Rn, tn
            q[c] = np.sqrt(rec["cost0"] / len(obs)), np.sqrt(rec["cost"] / len(obs)), rec["steps"]
    return (R, t, q, nu, st, recs) if trace else (R, t, q, nu, st)


def bootstrap(pt_ptr, cam_idx, xy, K, pose_threshold, n_hyp=512, seed=0, start_pair=None, min_points=12, max_rms=None, roots="roots",
              solver="chol"):
    """(R, t, X, info) as lib.initialization.bootstrap with ``pose_threshold`` (and no other threshold), on the host: the driver
    of tests/_bootstrap_ref.py with the calibrated registration below, and tests/_twoview_ref.py's plain relative_pose and
    triangulation.  ``K`` (m, 3, 3) projects to the units of xy."""
    R, t, X, info, _ = B.bootstrap(pt_ptr, cam_idx, xy, K, lambda pair: T.relative_pose(pt_ptr, cam_idx, xy, K, pair),
                                   register_robust(pt_ptr, cam_idx, xy, K, pose_threshold, min_points, n_hyp, seed, roots, solver),
                                   T.triangulate_plain, start_pair, max_rms)
    return R, t, X, {key: info[key] for key in B.ROBUST_KEYS}


def register_robust(pt_ptr, cam_idx, xy, K, threshold, min_points, n_hyp=512, seed=0, roots="roots", solver="chol"):
    """The registration step of tests/_bootstrap_ref.py with ``pose_threshold``: the calibrated robust registration of the
    unregistered cameras, ``most_inliers`` of them, the pose taken as returned."""
    pt_ptr, cam_idx, xy = np.asarray(pt_ptr), np.asarray(cam_idx), np.asarray(xy, np.float64).reshape(-1, 2)
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))

    def register(X, point_ok, camera_ok):
        todo = np.nonzero(~camera_ok)[0]
        ri = pose_robust(np.where(point_ok[:, None], X, 0.0), pt_ptr, cam_idx, xy, K, threshold, point_ok=point_ok, cameras=todo,
                         n_hyp=n_hyp, seed=seed, roots=roots, solver=solver)
        pick = B.most_inliers(ri, todo, cam_idx, point_ok[pt], min_points)
        if pick is None:
            return None
        i, c, sel, dropped = pick
        return c, ri["R"][i], ri["t"][i], sel, dropped

    return register
