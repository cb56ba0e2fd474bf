"""NumPy restatement of the robust triangulation entry point (include/mvba.h: mvba_triangulate_robust, mvba_triangulate_sample)
and of the driver that uses it (lib/initialization.py: bootstrap with ``triangulate_threshold``) -- the definitions written out
plainly on tests/_init_ref.py (camera_matrices, triangulate_point), tests/_ransac_ref.py (mix) and the two robust references.
Two host routes: ``linear`` = "eigh" or "svd" for the refits' linear step (as everywhere), ``rays`` = "adjugate" (the definition:
M^-1 by the adjugate) or "solve" (``np.linalg.solve``) for the viewing rays of the midpoint.  Test infrastructure only."""
import numpy as np

import _bootstrap_ref as B
import _init_ref as ref
import _ransac_ref as RR
import _resect_ransac_ref as QR
import _twoview_ref as T

REL_PIVOT = ref.REL_PIVOT
MAX_HYP = 4096  # csrc/mvba_tri_ransac.h: TR_MAX_HYP
MAX_ALT = 4     # outcomes of two Gauss-Newton decisions: alt_X, alt_quality are padded to it with NaN


def sample(seed, a, h, deg, n_hyp):
    """The observation numbers (i, j), i < j, of hypothesis h of point a with deg observations; (-1, -1) where the exhaustive
    table has no entry h."""
    n_pairs = deg * (deg - 1) // 2
    if n_pairs <= n_hyp:
        if h >= n_pairs:
            return -1, -1
        i, r = 0, h
        while r >= deg - 1 - i:
            r -= deg - 1 - i
            i += 1
        return i, i + 1 + r
    s = RR.mix(RR.mix(RR.mix(seed & RR.MASK) ^ ((a << 32) | a)) ^ h)
    idx = []
    while len(idx) < 2:
        s = RR.mix(s)
        j = ((s >> 32) * deg) >> 32
        if j not in idx:
            idx.append(j)
    return min(idx), max(idx)


def ray_directions(Pk, xy, rays="adjugate"):
    """Unit directions d = M^-1 (x, y, 1), M = P[:, :3], of the observations xy (n, 2) under their matrices Pk (n, 3, 4)."""
    M = Pk[:, :, :3]
    v = np.concatenate([xy, np.ones((len(xy), 1))], axis=1)
    with np.errstate(all="ignore"):
        if rays == "adjugate":
            adj = np.stack([np.cross(M[:, 1], M[:, 2]), np.cross(M[:, 2], M[:, 0]), np.cross(M[:, 0], M[:, 1])], axis=2)  # columns = cofactor rows
            det = np.einsum("ni,ni->n", M[:, 0], adj[:, :, 0])
            d = np.einsum("nij,nj->ni", adj, v) / det[:, None]
        else:
            d = np.stack([np.linalg.solve(Mk, vk) if abs(np.linalg.det(Mk)) > 0 else np.full(3, np.nan) for Mk, vk in zip(M, v)])
        return d / np.linalg.norm(d, axis=1, keepdims=True)


def midpoints(d, c, i, j):
    """(X (h, 3), NaN where degenerate) of the ray pairs (i[h], j[h]): directions d (n, 3), centres c (n, 3)."""
    with np.errstate(all="ignore"):
        d1, d2, b = d[i], d[j], c[j] - c[i]
        al = (d1 * d2).sum(axis=1)
        den = 1.0 - al * al
        b1, b2 = (b * d1).sum(axis=1), (b * d2).sum(axis=1)
        s, u = (b1 - al * b2) / den, (al * b1 - b2) / den
        X = 0.5 * (c[i] + s[:, None] * d1 + c[j] + u[:, None] * d2)
        good = (den > REL_PIVOT) & np.isfinite(X).all(axis=1)
    X[~good] = np.nan
    return X


def reprojection(Pk, xy, X):
    """(squared reprojection distances, depths P[2] . (X, 1)), each (..., n), of the point's observations under X (..., 3)."""
    with np.errstate(all="ignore"):
        p = np.einsum("nij,...j->...ni", Pk[:, :, :3], X) + Pk[:, :, 3]
        r = p[..., :2] / p[..., 2:3] - xy
        return (r * r).sum(axis=-1), p[..., 2]


TIE = 1e-12  # two costs of a Gauss-Newton step that agree to this (relative) are a tie: see refine_candidates


def refine_candidates(Pk, xy, X0, n_refine):
    """The Gauss-Newton steps of _init_ref.triangulate_point from its linear solution X0, replayed: a list of X, first the one
    its rule gives in this arithmetic (a step is taken only if it does not raise the cost: ``En <= E``), then what the rule gives
    when a decision whose two costs agree to TIE falls the other way.  Near convergence a step moves X by 1e-8 .. 1e-10 and the
    cost by the square of that, below the rounding of the cost itself -- a sum of 2 deg squares, of relative error about
    2 deg eps, 1e-14 at deg = 50, and another arithmetic (fused multiply-adds, another summation order) decides such a step
    differently.  TIE is 100 x that estimate (the MARGIN of every parity bound here).  Both outcomes are the cost's minimum to
    its resolution; they differ in X by the size of the step.  An implementation has to return one of them."""
    out = []

    def walk(X, E, H, g, steps):
        if steps == 0:
            return out.append(X)
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return out.append(X)
        Xn = X - np.linalg.solve(L.T, np.linalg.solve(L, g))
        En, Hn, gn = ref._eval(Pk, xy, Xn)
        take = bool(En <= E)
        for decision in ([take, not take] if abs(En - E) <= TIE * E else [take]):
            walk(Xn, En, Hn, gn, steps - 1) if decision else out.append(X)

    with np.errstate(all="ignore"):
        walk(X0, *ref._eval(Pk, xy, X0), n_refine)
    return out


def robust_triangulate_point(P, R, t, a, cams, xy, threshold, n_hyp, seed, n_refine, n_refit, linear="eigh", rays="adjugate"):
    """One point from its observations in list order.  A dict: X (3,), quality (3,), status, n_inliers, best, mask (deg,),
    hyp_count (H,), ``margin`` -- the smallest |d^2 / threshold^2 - 1| over every distance compared with the threshold --,
    ``Xmid`` (the best midpoint), ``alt_X``, ``alt_quality`` (MAX_ALT, 3) -- row 0 is (X, quality); further rows, NaN where there
    are none, are the other outcomes of ``n_ties`` tied Gauss-Newton decisions of the last kept refit (refine_candidates; n_refine
    <= 2) -- and the trace of the refit loop: ``n_accepted``, ``sizes`` (|I_0|, |I_1|, ... of X_best and of
    every refit that was evaluated, -1 padded to 1 + n_refit) and ``end`` -- "rejected", "solver", "exhausted", or "" for a
    point whose status is not 0."""
    deg, H, thr2 = len(cams), int(n_hyp), threshold * threshold
    nan3 = np.full(3, np.nan)
    out = {"X": nan3, "quality": nan3, "status": 1, "n_inliers": 0, "best": -1, "mask": np.zeros(deg, bool),
           "hyp_count": np.full(H, -1, np.int32), "margin": np.inf, "Xmid": nan3, "n_accepted": 0, "sizes": np.full(1 + n_refit, -1), "end": "",
           "alt_X": np.full((MAX_ALT, 3), np.nan), "alt_quality": np.full((MAX_ALT, 3), np.nan), "n_ties": 0}
    if deg < 2:
        return out
    Pk = P[cams]
    pairs = np.array([sample(seed, a, h, deg, H) for h in range(H)])
    listed = pairs[:, 0] >= 0
    Xh = np.full((H, 3), np.nan)
    Xh[listed] = midpoints(ray_directions(Pk, xy, rays), t[cams], pairs[listed, 0], pairs[listed, 1])
    ok = np.isfinite(Xh).all(axis=1)
    d2, depth = reprojection(Pk, xy, Xh)
    with np.errstate(all="ignore"):
        inl = (depth > 0) & (d2 <= thr2)
        if ok.any():
            out["margin"] = np.abs(d2[ok] / thr2 - 1.0).min()
    out["hyp_count"] = np.where(ok, inl.sum(axis=1), -1).astype(np.int32)
    best = int(np.argmax(out["hyp_count"]))
    if out["hyp_count"][best] < 0:
        out["status"] = 2
        return out
    out["best"] = best
    need = min(deg, 3)
    if out["hyp_count"][best] < need:
        out["status"] = 4
        return out
    mask, X, end, n_acc, cands = inl[best], Xh[best], "exhausted", 0, [Xh[best]]
    out["sizes"][0] = mask.sum()
    for r in range(1, n_refit + 1):
        Xr, _, st = ref.triangulate_point(P, R, t, cams[mask], xy[mask], n_refine, linear)
        if st != 0:
            end = "solver"
            break
        cr = refine_candidates(Pk[mask], xy[mask], ref.triangulate_point(P, R, t, cams[mask], xy[mask], 0, linear)[0], n_refine)
        assert cr[0].tobytes() == Xr.tobytes()  # (the replay is triangulate_point's own arithmetic)
        dr, zr = reprojection(Pk, xy, Xr)
        out["margin"] = min(out["margin"], np.abs(dr / thr2 - 1.0).min())
        new = (zr > 0) & (dr <= thr2)
        out["sizes"][r] = new.sum()
        if new.sum() < (need if r == 1 else mask.sum()):
            end = "rejected"
            break
        n_acc, mask, X, cands = n_acc + 1, new, Xr, cr
    ck = cams[mask]
    i, j = np.triu_indices(len(ck), 1)

    def quality(Y):
        ray = Y - t[ck]
        return np.array([np.sqrt(reprojection(Pk, xy, Y)[0][mask].sum() / mask.sum()), np.einsum("oi,oi->o", R[ck][:, :, 2], ray).min(),
                         np.arctan2(np.linalg.norm(np.cross(ray[i], ray[j]), axis=1), (ray[i] * ray[j]).sum(axis=1)).max()])

    # the outcomes of tied Gauss-Newton decisions in the last kept refit (refine_candidates): each must select the same inliers
    for Y in cands[1:]:
        dy, zy = reprojection(Pk, xy, Y)
        assert np.array_equal((zy > 0) & (dy <= thr2), mask)
    alt_X, alt_q = np.full((MAX_ALT, 3), np.nan), np.full((MAX_ALT, 3), np.nan)
    alt_X[:len(cands)], alt_q[:len(cands)] = cands, [quality(Y) for Y in cands]
    out.update(X=X, quality=quality(X), status=0, n_inliers=int(mask.sum()), mask=mask, Xmid=Xh[best], n_accepted=n_acc, end=end,
               alt_X=alt_X, alt_quality=alt_q, n_ties=len(cands) - 1)
    return out


def triangulate_robust(K, R, t, pt_ptr, cam_idx, xy, threshold, n_hyp=64, seed=0, n_refine=2, n_refit=2, linear="eigh", rays="adjugate"):
    """A dict of arrays over the points: X (N, 3), quality (N, 3), status, n_inliers, best (N,), hyp_count (N, H), inlier
    (n_obs,), margin (N,), Xmid (N, 3) and the refit trace n_accepted, sizes, end.  pt_ptr None: the dense grid, xy (N, m, 2)."""
    K, R, t = (np.asarray(v, np.float64) for v in (K, R, t))
    if pt_ptr is None:
        xy = np.asarray(xy, np.float64)
        pt_ptr, cam_idx = ref.dense_list(xy.shape[0], K.shape[0])
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    P = ref.camera_matrices(K, R, t)
    res, inlier = [], np.zeros(len(xy), bool)
    for a in range(len(pt_ptr) - 1):
        o = slice(pt_ptr[a], pt_ptr[a + 1])
        r = robust_triangulate_point(P, R, t, a, np.asarray(cam_idx[o]), xy[o], threshold, n_hyp, seed, n_refine, n_refit, linear, rays)
        inlier[o] = r["mask"]
        res.append(r)
    keys = ("X", "quality", "status", "n_inliers", "best", "hyp_count", "margin", "Xmid", "n_accepted", "sizes", "end", "alt_X", "alt_quality",
            "n_ties")
    out = {key: np.array([r[key] for r in res]) for key in keys}
    out["status"], out["n_inliers"], out["best"] = (out[k].astype(np.int32) for k in ("status", "n_inliers", "best"))
    out["inlier"] = inlier
    for v in out.values():
        v.setflags(write=False)
    return out


def bootstrap(pt_ptr, cam_idx, xy, K, ransac_threshold=None, resect_threshold=None, triangulate_threshold=None, n_hyp=512, seed=0,
              start_pair=None, min_points=12, max_rms=None, linear="eigh", rays="adjugate"):
    """(R, t, X, info) as lib.initialization.bootstrap with any of its three thresholds, on the host: the driver of
    tests/_bootstrap_ref.py with, for each threshold given, the robust step of tests/_ransac_ref.py (the first F),
    tests/_resect_ransac_ref.py (every later camera) and the robust triangulation above, and tests/_twoview_ref.py's plain step
    otherwise.  ``K`` (m, 3, 3) projects to the units of xy.  ``info`` also has ``margin``: the
    smallest one over every robust triangulation of the run (inf without ``triangulate_threshold``), and ``alt_X`` (N, a, 3): the
    last round's points with the other outcomes of tied Gauss-Newton decisions (refine_candidates), in the output frame."""
    if ransac_threshold is None:
        def start(pair):
            return T.relative_pose(pt_ptr, cam_idx, xy, K, pair)
    else:
        def start(pair):
            return RR.relative_pose(pt_ptr, cam_idx, xy, K, pair, ransac_threshold, n_hyp, seed, linear=linear)
    if resect_threshold is None:
        register = T.register_plain(pt_ptr, cam_idx, xy, K, min_points)
    else:
        register = QR.register_robust(pt_ptr, cam_idx, xy, K, resect_threshold, min_points, n_hyp, seed, linear)

    def triangulate(Kr, Rr, tr, ptr, cam, z):
        """With the threshold the robust triangulation above; ``extras``: the points before the keep rule with the other outcomes
        of tied decisions, and the round's margin."""
        if triangulate_threshold is None:
            X, q, s, used, _ = T.triangulate_plain(Kr, Rr, tr, ptr, cam, z)
            return X, q, s, used, {"alt_X": X[:, None, :]}  # (a view: it gets the keep rule's NaN with X)
        ti = triangulate_robust(Kr, Rr, tr, ptr, cam, z, triangulate_threshold, min(n_hyp, MAX_HYP), seed, 2, 2, linear, rays)
        return ti["X"].copy(), ti["quality"], ti["status"], ti["inlier"], {"alt_X": ti["alt_X"], "margin": ti["margin"].min()}

    R, t, X, info, trace = B.bootstrap(pt_ptr, cam_idx, xy, K, start, register, triangulate, start_pair, max_rms)
    R0, t0, s = trace["frame"]
    alt = trace["extras"][-1]["alt_X"] if trace["extras"] else trace["start"][2][:, None, :]
    info.update(margin=min([np.inf] + [e["margin"] for e in trace["extras"] if "margin" in e]), alt_X=((alt - t0) @ R0) / s)
    return R, t, X, info
