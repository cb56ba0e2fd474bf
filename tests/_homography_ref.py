"""NumPy restatement of the planar two-view entry points (include/mvba.h: mvba_homography_robust, mvba_homography_sample) and of
the drivers that use them (lib/initialization.py: homography_pose_candidates, relative_pose and bootstrap with ``model``) --
the definitions written out plainly on tests/_ransac_ref.py and tests/_twoview_ref.py, with two routes to every linear
solution: the closed form / ``np.linalg.eigh`` the library states, and the SVD of the stacked rows.  Test infrastructure only."""
import numpy as np

import _bootstrap_ref as B
import _init_ref as ref
import _pose_ransac_ref as PR
import _ransac_ref as RR
import _twoview_ref as T

REL_PIVOT = T.REL_PIVOT


def sample(seed, k, l, h, n):
    """The 4 distinct indices below n of hypothesis h of pair (k, l): the first four draws of _ransac_ref.sample's generator."""
    s = RR.mix(RR.mix(RR.mix(seed & RR.MASK) ^ ((k << 32) | l)) ^ h)
    idx = []
    while len(idx) < 4:
        s = RR.mix(s)
        j = ((s >> 32) * n) >> 32
        if j not in idx:
            idx.append(j)
    return np.array(idx, np.int64)


def det3(a, b, c):
    """det [(a, 1) (b, 1) (c, 1)] in the library's order of operations."""
    return a[0] * (b[1] - c[1]) - b[0] * (a[1] - c[1]) + c[0] * (a[1] - b[1])


def adjugate(M):
    m = M.reshape(9)
    return np.array([m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                     m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                     m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]).reshape(3, 3)


def triple_pivot(p):
    """The smallest |det [p_a p_b p_c]| / (|p_a| |p_b| |p_c|) over the four triples of the four points p (4, 2)."""
    nr = np.sqrt((p * p).sum(axis=1) + 1.0)
    return min(abs(det3(p[a], p[b], p[c])) / (nr[a] * nr[b] * nr[c]) for a, b, c in ((0, 1, 2), (3, 1, 2), (0, 3, 2), (0, 1, 3)))


def basis(p):
    """B = [l1 p1, l2 p2, l3 p3] with [p1 p2 p3] l = p4 by Cramer's rule, the common 1 / det left out."""
    lam = np.array([det3(p[3], p[1], p[2]), det3(p[0], p[3], p[2]), det3(p[0], p[1], p[3])])
    return np.vstack([p[:3].T, np.ones(3)]) * lam


def rows(a, b):
    """The two DLT rows per correspondence b ~ H a, stacked (2 n, 9): first rows, then second rows."""
    n, z, one = len(a), np.zeros(len(a)), np.ones(len(a))
    r1 = np.stack([a[:, 0], a[:, 1], one, z, z, z, -b[:, 0] * a[:, 0], -b[:, 0] * a[:, 1], -b[:, 0]], axis=1)
    r2 = np.stack([z, z, z, a[:, 0], a[:, 1], one, -b[:, 1] * a[:, 0], -b[:, 1] * a[:, 1], -b[:, 1]], axis=1)
    return np.concatenate([r1, r2]).reshape(2 * n, 9)


def _signed(M):
    return -M if M[2, 2] < 0 else M


def four_point(pk, pl, route="closed"):
    """(H^, H^^-1 up to scale) of four normalised correspondences, each signed so that its [2][2] entry is positive (the third
    coordinate at the origin, the centroid of the normalised points).  "closed": B_l adj(B_k) and B_k adj(B_l); "svd": the null
    vector of the stacked 8 x 9 rows, and its adjugate."""
    if route == "closed":
        Bk, Bl = basis(pk), basis(pl)
        return _signed(Bl @ adjugate(Bk)), _signed(Bk @ adjugate(Bl))
    Hh = np.linalg.svd(rows(pk, pl), full_matrices=True)[2][8].reshape(3, 3)
    return _signed(Hh), _signed(adjugate(Hh))


def transfer(M, x, tx):
    """(a, w): (u - tx w)^2 + (v - ty w)^2 and w for (u, v, w) = M (x, 1); M (..., 3, 3), x and tx (n, 2) -> (..., n)."""
    hx = np.c_[x, np.ones(len(x))]
    p = np.einsum("...ij,nj->...ni", M, hx)
    eu, ev = p[..., 0] - tx[:, 0] * p[..., 2], p[..., 1] - tx[:, 1] * p[..., 2]
    return eu * eu + ev * ev, p[..., 2]


def inlier_test(Hf, Hb, xk, xl, thr2, one_way=False):
    """(inlier (..., n), d2 (..., n), guard): the library's test, division-free -- w > 0 and a <= thr^2 w^2, both ways -- the mean
    of the two squared transfer distances, and the guard: the smallest |a / (thr^2 w^2) - 1| over every comparison made, and
    over those that pass it the smallest |w| relative to |h6 x| + |h7 y| + |h8|, the size of its terms (a w of the other sign
    would flip them).
    ``one_way``: the altered copy that tests k -> l only (test_homography_cpu.py)."""
    with np.errstate(all="ignore"):
        af, wf = transfer(Hf, xk, xl)
        ab, wb = transfer(Hb, xl, xk)
        okf, okb = (wf > 0) & (af <= thr2 * wf * wf), (wb > 0) & (ab <= thr2 * wb * wb)
        d2 = 0.5 * (af / (wf * wf) + ab / (wb * wb))
        guard = np.inf
        for a, w, M, x in ((af, wf, Hf, xk), (ab, wb, Hb, xl)):
            fin = np.isfinite(a) & np.isfinite(w)
            if not fin.any():
                continue
            ra = np.abs(a / (thr2 * w * w) - 1.0)
            guard = min(guard, np.nanmin(np.where(fin, ra, np.inf)))
            passes = fin & (a <= thr2 * w * w)
            if passes.any():
                rw = np.abs(w) / (np.abs(M[..., 2, 0, None] * x[:, 0]) + np.abs(M[..., 2, 1, None] * x[:, 1]) + np.abs(M[..., 2, 2, None]))
                guard = min(guard, rw[passes].min())
    return (okf if one_way else okf & okb), d2, guard


def unit(M):
    M = M / np.linalg.norm(M)
    return -M if M.flat[np.argmax(np.abs(M))] < 0 else M


def mask_parts(H, ck, cl):
    """(+-H, +-adj(H)): each with the sign that makes the third coordinate positive at the centroid it is applied to."""
    A = adjugate(H)
    return (-H if H[2] @ np.r_[ck, 1.0] < 0 else H), (-A if A[2] @ np.r_[cl, 1.0] < 0 else A)


def homography(xk, xl, linear="eigh"):
    """(H (3, 3), ratio, status, c_k, c_l) of the normalised DLT over all the points given: |H| = 1, largest entry positive."""
    nanH = np.full((3, 3), np.nan)
    with np.errstate(all="ignore"):
        ck, sk = ref.hartley(xk)
        cl, sl = ref.hartley(xl)
        r = rows(sk * (xk - ck), sl * (xl - cl))
        if not np.isfinite(r).all():
            return nanH, np.nan, 2, ck, cl
        if linear == "eigh":
            w, V = np.linalg.eigh(r.T @ r)
            h = V[:, 0]
        else:
            _, s, Vt = np.linalg.svd(r, full_matrices=len(r) < 9)
            w, h = np.concatenate([s, np.zeros(9 - len(s))])[::-1] ** 2, Vt[8]
    if not w[1] > REL_PIVOT * w[8]:
        return nanH, w[0] / w[1], 2, ck, cl
    H = np.linalg.inv(T.hartley_T(cl, sl)) @ h.reshape(3, 3) @ T.hartley_T(ck, sk)
    if not np.isfinite(H).all():
        return nanH, w[0] / w[1], 2, ck, cl
    return unit(H), w[0] / w[1], 0, ck, cl


def hypotheses(xk, xl, k, l, seed, hs, route="closed", no_degeneracy_rule=False):
    """(Hf, Hb (len(hs), 3, 3), pivot (len(hs),)) of the hypotheses ``hs`` in the units of xy; NaN where degenerate."""
    n = len(xk)
    ck, sk = ref.hartley(xk)
    cl, sl = ref.hartley(xl)
    Tk, Tl = T.hartley_T(ck, sk), T.hartley_T(cl, sl)
    a, b = sk * (xk - ck), sl * (xl - cl)
    Hf, Hb, pivot = np.full((len(hs), 3, 3), np.nan), np.full((len(hs), 3, 3), np.nan), np.full(len(hs), np.nan)
    for i, h in enumerate(hs):
        idx = sample(seed, k, l, int(h), n)
        pk, pl = a[idx], b[idx]
        if not (np.isfinite(pk).all() and np.isfinite(pl).all()):
            continue
        pivot[i] = min(triple_pivot(pk), triple_pivot(pl))
        if not pivot[i] > REL_PIVOT and not no_degeneracy_rule:
            continue
        hf, hb = four_point(pk, pl, route)
        F, B = np.linalg.inv(Tl) @ hf @ Tk, np.linalg.inv(Tk) @ hb @ Tl
        if np.isfinite(F).all() and np.isfinite(B).all():
            Hf[i], Hb[i] = F, B
    return Hf, Hb, pivot


def robust_homography(xk, xl, k, l, threshold, n_hyp, seed, n_refit, route="closed", one_way=False, no_degeneracy_rule=False):
    """One pair.  A dict as _ransac_ref.robust_fundamental's, with H for F; ``margin`` is the guard of inlier_test over every
    test made; ``route``: "closed" (closed-form hypotheses, eigh refits) or "svd" (SVD for both)."""
    n, nh, thr2 = len(xk), int(n_hyp), threshold * threshold
    out = {"H": np.full((3, 3), np.nan), "quality": np.full(2, np.nan), "status": 1, "n_inliers": 0, "best": -1, "mask": np.zeros(n, bool),
           "hyp_count": np.full(nh, -1, np.int32), "margin": np.inf, "pivot": np.full(nh, np.nan), "n_accepted": 0, "n_changed": 0, "end": ""}
    if n < 4:
        return out
    with np.errstate(all="ignore"):
        Hf, Hb, out["pivot"] = hypotheses(xk, xl, k, l, seed, range(nh), route, no_degeneracy_rule)
        ok = np.isfinite(Hf).all(axis=(1, 2))
        inl, d2, out["margin"] = inlier_test(Hf, Hb, xk, xl, thr2, one_way)
        out["hyp_count"] = np.where(ok, inl.sum(axis=1), -1).astype(np.int32)
    best = int(np.argmax(out["hyp_count"]))
    if out["hyp_count"][best] < 0:
        out["status"] = 2
        return out
    out["best"] = best
    if out["hyp_count"][best] < 4:
        out["status"] = 4
        return out
    mask, dd = inl[best], d2[best]
    H, ratio, end, n_acc, n_chg = unit(Hf[best]), 0.0, "exhausted", 0, 0
    for _ in range(n_refit):
        Hr, rt, st, ck, cl = homography(xk[mask], xl[mask], "eigh" if route == "closed" else "svd")
        if st != 0:
            end = "solver"
            break
        m0, m1 = mask_parts(Hr, ck, cl)
        ir, dr, g = inlier_test(m0, m1, xk, xl, thr2, one_way)
        out["margin"] = min(out["margin"], g)
        if ir.sum() < mask.sum():
            end = "rejected"
            break
        n_acc, n_chg = n_acc + 1, n_chg + int(not np.array_equal(ir, mask))
        H, ratio, mask, dd = Hr, rt, ir, dr
    out.update(H=H, quality=np.array([np.sqrt(dd[mask].sum() / mask.sum()), ratio]), status=0, n_inliers=int(mask.sum()), mask=mask,
               n_accepted=n_acc, n_changed=n_chg, end=end)
    return out


def homography_robust(pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hyp=512, seed=0, n_refit=2, route="closed", **alter):
    """A dict of arrays over the pairs, as _ransac_ref.two_view_robust's with H for F."""
    pt_ptr, cam_idx, xy = T._list(pt_ptr, cam_idx, xy, n_images)
    pairs = np.asarray(pairs).reshape(-1, 2)
    N, res, ns = len(pt_ptr) - 1, [], []
    inl = np.zeros((len(pairs), N), bool)
    for i, (k, l) in enumerate(pairs):
        ids, xk, xl = T.shared(pt_ptr, cam_idx, xy, k, l)
        r = robust_homography(xk, xl, int(k), int(l), threshold, n_hyp, seed, n_refit, route, **alter)
        inl[i, ids[r["mask"]]] = True
        res.append(r)
        ns.append(len(ids))
    out = {key: np.array([r[key] for r in res]) for key in ("H", "quality", "n_inliers", "best", "status", "hyp_count", "margin", "pivot",
                                                            "n_accepted", "n_changed", "end")}
    out.update(n_shared=np.array(ns, np.int64), inlier=inl)
    for v in out.values():
        v.setflags(write=False)
    return out


def pose_candidates(Hn, route="eigh"):
    """lib.initialization.homography_pose_candidates; "svd": the right singular vectors instead of the eigenvectors of Hn^T Hn."""
    if not np.isfinite(Hn).all():
        return []
    sv = np.linalg.svd(Hn, compute_uv=False)
    if not sv[1] > 0 or sv[0] - sv[2] <= 1e-12 * sv[1]:
        return []
    Hn = Hn / sv[1] * np.sign(np.linalg.det(Hn))
    if route == "eigh":
        w, V = np.linalg.eigh(Hn.T @ Hn)
        v1, v2, v3, s1, s3 = V[:, 2], V[:, 1], V[:, 0], max(w[2], 1.0), min(w[0], 1.0)
    else:
        _, s, Vt = np.linalg.svd(Hn)
        v1, v2, v3, s1, s3 = Vt[0], Vt[1], Vt[2], max(s[0] ** 2, 1.0), min(s[2] ** 2, 1.0)
    v1, v2, v3 = (v if v[np.argmax(np.abs(v))] > 0 else -v for v in (v1, v2, v3))
    out = []
    for sg in (1.0, -1.0):
        u = (np.sqrt(1.0 - s3) * v1 + sg * np.sqrt(s1 - 1.0) * v3) / np.sqrt(s1 - s3)
        U = np.stack([v2, u, np.cross(v2, u)], axis=1)
        W = np.stack([Hn @ v2, Hn @ u, np.cross(Hn @ v2, Hn @ u)], axis=1)
        Rrel, nn = W @ U.T, np.cross(v2, u)
        tau = (Hn - Rrel) @ nn
        d = 1.0 / np.linalg.norm(tau)
        for sgn in (1.0, -1.0):
            out.append((Rrel.T, -sgn * d * Rrel.T @ tau, sgn * nn / d))
    return out


def closest_candidate(cands, Rg, tg):
    """(index, max-abs error over R and t) of the candidate closest to (Rg, tg)."""
    err = [max(np.abs(R - Rg).max(), np.abs(t - tg).max()) for R, t, _ in cands]
    return int(np.argmin(err)), float(np.min(err))


def homography_pose(pt_ptr, cam_idx, xy, K, pair, threshold, n_hyp=512, seed=0, n_refine=2, route="closed", candidate=None):
    """(R, t, X, info) as lib.initialization.relative_pose(model="homography", homography_threshold=threshold)."""
    k, l = pair
    n = len(pt_ptr) - 1
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ids, xk, xl = T.shared(pt_ptr, cam_idx, xy, k, l)
    r = robust_homography(xk, xl, int(k), int(l), threshold, n_hyp, seed, 2, route)
    inlier = np.zeros(n, bool)
    inlier[ids[r["mask"]]] = True
    info = {"n_front": np.zeros(4, np.int64), "rms": np.full(4, np.inf), "status": int(r["status"]), "H": r["H"], "n_shared": len(ids),
            "inlier": inlier, "n_inliers": r["n_inliers"], "n_inliers_H": r["n_inliers"], "quality": np.full((n, 3), np.nan),
            "model": "homography", "candidates": [], "ambiguous": False, "plane": None}
    if r["status"] != 0:
        return (*T.no_pose(n), info)
    ids, xk, xl = ids[r["mask"]], xk[r["mask"]], xl[r["mask"]]
    cands = pose_candidates(np.linalg.solve(K[l], r["H"]) @ K[k], "eigh" if route == "closed" else "svd")
    info["candidates"] = cands
    if not cands:
        info["status"] = 3
        return (*T.no_pose(n), info)
    R, t, X, best = T.choose_candidate(K, pair, cands, ids, xk, xl, info, n_refine, by_rms=True, candidate=candidate)
    if best is not None:
        nn = cands[best][2]
        info.update(plane=(nn / np.linalg.norm(nn), 1.0 / np.linalg.norm(nn)), best_candidate=best)
    return R, t, X, info


def relative_pose(pt_ptr, cam_idx, xy, K, pair, threshold, model="auto", homography_threshold=None, planar_ratio=0.8, n_hyp=512, seed=0,
                  route="closed"):
    """(R, t, X, info) as lib.initialization.relative_pose with ``ransac_threshold`` = threshold and ``model``; info carries
    ``ratio`` = n_inliers_H / n_inliers_F where both were fitted."""
    lin = "eigh" if route == "closed" else "svd"
    if model == "fundamental":
        out = RR.relative_pose(pt_ptr, cam_idx, xy, K, pair, threshold, n_hyp, seed, linear=lin)
        out[3]["model"] = "fundamental"
        return out
    thr_h = threshold if homography_threshold is None else homography_threshold
    if model == "homography":
        return homography_pose(pt_ptr, cam_idx, xy, K, pair, thr_h, n_hyp, seed, route=route)
    k, l = pair
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    _, xk, xl = T.shared(pt_ptr, cam_idx, xy, k, l)
    rf = RR.robust_fundamental(xk, xl, int(k), int(l), threshold, n_hyp, seed, 2, lin)
    rh = robust_homography(xk, xl, int(k), int(l), thr_h, n_hyp, seed, 2, route)
    ratio = rh["n_inliers"] / rf["n_inliers"] if rf["n_inliers"] else np.inf
    planar = rh["status"] == 0 and (rf["status"] != 0 or rh["n_inliers"] >= planar_ratio * rf["n_inliers"])
    if planar:
        out = homography_pose(pt_ptr, cam_idx, xy, K, pair, thr_h, n_hyp, seed, route=route)
    else:
        out = RR.relative_pose(pt_ptr, cam_idx, xy, K, pair, threshold, n_hyp, seed, linear=lin)
        out[3].update(model="fundamental", H=rh["H"], n_inliers_H=rh["n_inliers"])
    out[3].update(ratio=ratio, n_inliers_F=rf["n_inliers"])
    return out


def hypothesis_counts(xk, xl, k, l, threshold, seed, hs, route="closed"):
    """(counts, guard, pivot) of the entries ``hs`` of the pair's count table alone (a hypothesis depends on (seed, k, l, h))."""
    if len(xk) < 4:
        return np.full(len(hs), -1, np.int32), np.inf, np.full(len(hs), np.nan)
    with np.errstate(all="ignore"):
        Hf, Hb, pivot = hypotheses(xk, xl, k, l, seed, hs, route)
        ok = np.isfinite(Hf).all(axis=(1, 2))
        inl, _, guard = inlier_test(Hf, Hb, xk, xl, threshold * threshold)
    return np.where(ok, inl.sum(axis=1), -1).astype(np.int32), guard, pivot


def bootstrap(pt_ptr, cam_idx, xy, K, threshold, pose_threshold, model="auto", n_hyp=512, seed=0, route="closed", start_pair=None, min_points=12,
              max_rms=None, roots="roots", solver="chol"):
    """(R, t, X, info) as lib.initialization.bootstrap(model=, ransac_threshold=threshold, pose_threshold=): the driver of
    tests/_bootstrap_ref.py with the relative_pose above as its start step, tests/_pose_ransac_ref.py's registration and the plain
    triangulation; with an ``ambiguous`` start the WHOLE driver runs under each of the two candidates and the one whose first
    registered camera has more inliers is kept (the first on a tie) -- the library decides by the first round alone.  info gains
    ``model`` and ``ambiguous``."""
    register = PR.register_robust(pt_ptr, cam_idx, xy, K, pose_threshold, min_points, n_hyp, seed, roots, solver)

    def run(cand):
        """The driver from relative_pose's own choice (None) or from candidate ``cand``, and the start step's info."""
        def start(pair):
            if cand is None:
                return relative_pose(pt_ptr, cam_idx, xy, K, pair, threshold, model, n_hyp=n_hyp, seed=seed, route=route)
            return homography_pose(pt_ptr, cam_idx, xy, K, pair, threshold, n_hyp, seed, route=route, candidate=cand)
        R, t, X, info, trace = B.bootstrap(pt_ptr, cam_idx, xy, K, start, register, T.triangulate_plain, start_pair, max_rms)
        return (R, t, X, {key: info[key] for key in B.ROBUST_KEYS}), trace["start"][3]

    out, pi = run(None)
    if pi.get("ambiguous"):
        nf, b = pi["n_front"], pi["best_candidate"]
        other = [c for c in range(4) if c != b and nf[c] >= nf[b]][0]
        alt, po = run(other)

        def first(o):  # the inliers of the first camera registered after the pair
            c = o[3]["order"][2] if len(o[3]["order"]) > 2 else None
            return 0 if c is None else int((o[3]["inlier"] & (np.asarray(cam_idx) == c)).sum())
        if po["status"] == 0 and first(alt) > first(out):
            out = alt
    out[3].update(model=pi["model"], ambiguous=bool(pi.get("ambiguous")))
    return out
