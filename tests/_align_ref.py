"""NumPy restatement of the similarity-alignment entry points (include/mvba.h: mvba_align_robust, mvba_align, mvba_align_sample):
the sampler, the hypotheses, the counts, the arg-max with the lowest h on ties, the masks, the refits and the accept rule written
out plainly, with two routes to every solve: "horn" (``np.linalg.eigh`` of Horn's 4 x 4 matrix, what the library states) and "svd"
(Umeyama: the SVD of the 3 x 3 cross-covariance with the determinant fix).  Test infrastructure only."""
import numpy as np

import _ransac_ref as RR

REL_PIVOT = 1e-12  # csrc/mvba_ransac_host.h: INIT_REL_PIVOT
ROUTES = ("horn", "svd")


def rs_mix(x):
    x = (x + 0x9E3779B97F4A7C15) & RR.MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & RR.MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & RR.MASK
    return x ^ (x >> 31)


def rs_sample(seed, k, l, h, n, ns):
    """The ``ns`` distinct indices below n of hypothesis h of item (k, l): csrc/mvba_ransac.h's generator."""
    s = rs_mix(rs_mix(rs_mix(seed & RR.MASK) ^ ((k << 32) | l)) ^ h)
    idx = []
    while len(idx) < ns:
        s = rs_mix(s)
        j = ((s >> 32) * n) >> 32
        if j not in idx:
            idx.append(j)
    return np.array(idx, np.int64)


def sample(seed, h, n):
    """The 3 distinct indices below n of hypothesis h."""
    return rs_sample(seed, 0, 0, h, n, 3)


def horn_matrix(C):
    """Horn's symmetric 4 x 4 matrix of the cross-covariance C = sum y_c x_c^T (S[a][b] = sum x_c[a] y_c[b] = C[b][a])."""
    S = C.T
    return np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                     [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                     [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                     [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])


def quaternion_rotation(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def solve(mx, my, sxx, syy, C, with_scale=True, route="horn"):
    """(sim13, gap, status) from the centred moments: sim13 = (s, Q row-major, tau), gap = (l1 - l2) / l1 of the two largest
    eigenvalues of Horn's matrix; status 2 (sim13 NaN) where align_solve refuses."""
    nan = np.full(13, np.nan)
    with np.errstate(all="ignore"):
        if not (np.isfinite(C).all() and np.isfinite(sxx) and np.isfinite(syy) and sxx > 0 and syy > 0):
            return nan, np.nan, 2
        if route == "horn":
            w, V = np.linalg.eigh(horn_matrix(C))
            l1, l2, Q = w[3], w[2], quaternion_rotation(V[:, 3])
            num = (Q * C).sum()
        else:
            U, sv, Vt = np.linalg.svd(C)
            d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0
            Q = U @ np.diag([1.0, 1.0, d]) @ Vt
            l1, l2 = sv[0] + sv[1] + d * sv[2], sv[0] - sv[1] - d * sv[2]
            num = l1
        if not l1 > 0:
            return nan, np.nan, 2
        gap = (l1 - l2) / l1
        if not gap > REL_PIVOT:
            return nan, gap, 2
        s = num / sxx if with_scale else 1.0
        sim = np.concatenate([[s], Q.ravel(), my - s * Q @ mx])
        if not (np.isfinite(sim).all() and s > 0):
            return nan, gap, 2
    return sim, gap, 0


def fit(x, y, with_scale=True, route="horn"):
    """(sim13, gap, status, spread) of the least-squares similarity y ~ s Q x + tau over all the rows given; spread = sum |x_c|^2 /
    count."""
    mx, my = x.mean(axis=0), y.mean(axis=0)
    xc, yc = x - mx, y - my
    sxx = (xc * xc).sum()
    sim, gap, st = solve(mx, my, sxx, (yc * yc).sum(), yc.T @ xc, with_scale, route)
    return sim, gap, st, sxx / len(x)


def pivot(p):
    """|(p1 - p0) x (p2 - p0)|^2 / (|p1 - p0|^2 |p2 - p0|^2) of a triple p (3, 3)."""
    a, b = p[1] - p[0], p[2] - p[0]
    c = np.cross(a, b)
    with np.errstate(all="ignore"):
        return (c @ c) / ((a @ a) * (b @ b))


def hypotheses(x, y, seed, hs, with_scale=True, route="horn"):
    """(sim (len(hs), 13), pivot (len(hs),)): the hypotheses ``hs`` over the usable rows; NaN where degenerate."""
    n = len(x)
    sims, piv = np.full((len(hs), 13), np.nan), np.full(len(hs), np.nan)
    for i, h in enumerate(hs):
        idx = sample(seed, int(h), n)
        piv[i] = min(pivot(x[idx]), pivot(y[idx]))
        if not piv[i] > REL_PIVOT:
            continue
        sim, _, st, _ = fit(x[idx], y[idx], with_scale, route)
        if st == 0:
            sims[i] = sim
    return sims, piv


def residual2(sim, x, y):
    """|s Q x + tau - y|^2; sim (..., 13), x and y (n, 3) -> (..., n)."""
    sim = np.asarray(sim)
    sQ = sim[..., :1, None] * sim[..., 1:10].reshape(sim.shape[:-1] + (3, 3))
    d = np.einsum("...ij,nj->...ni", sQ, x) + sim[..., None, 10:13] - y
    return (d * d).sum(axis=-1)


def inlier_test(sim, x, y, thr2):
    """(inlier (..., n), d2 (..., n), guard): d2 <= thr^2 (NaN fails), and the smallest |d2 / thr^2 - 1| over every decision made
    with a finite d2."""
    with np.errstate(all="ignore"):
        d2 = residual2(sim, x, y)
        r = np.abs(d2 / thr2 - 1.0)
        fin = np.isfinite(d2)
        guard = r[fin].min() if fin.any() else np.inf
        return d2 <= thr2, d2, guard


def usable(src, dst, ok=None):
    u = np.isfinite(src).all(axis=1) & np.isfinite(dst).all(axis=1)
    return u if ok is None else u & (np.asarray(ok) != 0)


def decompose(sim):
    return sim[0], sim[1:10].reshape(3, 3), sim[10:13]


def align_robust(src, dst, threshold, ok=None, with_scale=True, n_hyp=512, seed=0, n_refit=2, route="horn"):
    """A dict with the outputs of mvba_align_robust (``sim13``; ``inlier`` over the input rows) and, beside them, ``margin`` (the
    guard of inlier_test over every test made), ``pivot`` per hypothesis, ``n_accepted`` and ``end``."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    u = usable(src, dst, ok)
    x, y, ids = src[u], dst[u], np.nonzero(u)[0]
    n, nh, thr2 = len(x), int(n_hyp), threshold * threshold
    out = {"sim13": np.full(13, np.nan), "quality": np.full(3, np.nan), "status": 1, "n_usable": n, "n_inliers": 0, "best": -1,
           "inlier": np.zeros(len(src), bool), "hyp_count": np.full(nh, -1, np.int32), "margin": np.inf, "pivot": np.full(nh, np.nan),
           "n_accepted": 0, "end": ""}
    if n < 3:
        return out
    sims, out["pivot"] = hypotheses(x, y, seed, range(nh), with_scale, route)
    good = np.isfinite(sims).all(axis=1)
    inl, d2, out["margin"] = inlier_test(sims, x, y, thr2)
    out["hyp_count"] = np.where(good, inl.sum(axis=1), -1).astype(np.int32)
    best = int(np.argmax(out["hyp_count"]))  # (the first of equals)
    if out["hyp_count"][best] < 0:
        out["status"] = 2
        return out
    out["best"] = best
    if out["hyp_count"][best] < 3:
        out["status"] = 4
        return out
    mask, dd, sim, gap, end, n_acc = inl[best], d2[best], sims[best], 0.0, "exhausted", 0
    for r in range(n_refit):
        sr, gr, st, _ = fit(x[mask], y[mask], with_scale, route)
        if st != 0:
            end = "solver"
            break
        ir, dr, g = inlier_test(sr, x, y, thr2)
        out["margin"] = min(out["margin"], g)
        if ir.sum() < (3 if r == 0 else mask.sum()):
            end = "rejected"
            break
        n_acc, sim, gap, mask, dd = n_acc + 1, sr, gr, ir, dr
    xm = x[mask] - x[mask].mean(axis=0)
    out["inlier"][ids[mask]] = True
    out.update(sim13=sim, quality=np.array([np.sqrt(dd[mask].sum() / mask.sum()), gap, (xm * xm).sum() / mask.sum()]), status=0,
               n_inliers=int(mask.sum()), n_accepted=n_acc, end=end)
    return out


def hypothesis_counts(src, dst, threshold, seed, hs, with_scale=True, route="horn"):
    """(counts, guard, pivot) of the hypotheses ``hs`` alone (all rows usable)."""
    sims, piv = hypotheses(src, dst, seed, hs, with_scale, route)
    inl, _, guard = inlier_test(sims, src, dst, threshold * threshold)
    return np.where(np.isfinite(sims).all(axis=1), inl.sum(axis=1), -1).astype(np.int32), guard, piv


def align(src, dst, ok=None, with_scale=True, route="horn"):
    """A dict with the outputs of mvba_align: ``sim13``, ``quality`` (3,), ``n_usable``, ``status``."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    u = usable(src, dst, ok)
    x, y = src[u], dst[u]
    out = {"sim13": np.full(13, np.nan), "quality": np.full(3, np.nan), "n_usable": int(u.sum()), "status": 1}
    if len(x) < 3:
        return out
    sim, gap, st, spread = fit(x, y, with_scale, route)
    out["status"] = st
    if st == 0:
        out.update(sim13=sim, quality=np.array([np.sqrt(residual2(sim, x, y).sum() / len(x)), gap, spread]))
    return out


def transform(sim, X=None, R=None, t=None):
    """transform_reconstruction, restated: (X', R', t')."""
    s, Q, tau = decompose(np.asarray(sim))
    return (None if X is None else s * X @ Q.T + tau, None if R is None else Q @ R, None if t is None else s * t @ Q.T + tau)


def inverse(sim):
    """The similarity that undoes ``sim``: x = (1 / s) Q^T (y - tau)."""
    s, Q, tau = decompose(np.asarray(sim))
    return np.concatenate([[1.0 / s], Q.T.ravel(), -(Q.T @ tau) / s])
