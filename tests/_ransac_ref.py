"""NumPy restatement of the robust two-view entry point (include/mvba.h: mvba_two_view_robust, mvba_ransac_sample) and of the
drivers that use it (lib/initialization.py: relative_pose and bootstrap with ``ransac_threshold``) -- the definitions written
out plainly on tests/_twoview_ref.py, with ``np.linalg.eigh`` (or the SVD of the stacked rows) where the device runs its own
Jacobi.  Test infrastructure only."""
import numpy as np

import _bootstrap_ref as B
import _init_ref as ref
import _twoview_ref as T

MASK = (1 << 64) - 1


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def sample(seed, k, l, h, n):
    """The 8 distinct indices below n of hypothesis h of pair (k, l)."""
    s = mix(mix(mix(seed & MASK) ^ ((k << 32) | l)) ^ h)
    idx = []
    while len(idx) < 8:
        s = mix(s)
        j = ((s >> 32) * n) >> 32
        if j not in idx:
            idx.append(j)
    return np.array(idx, np.int64)


def sampson_d2(F, xk, xl):
    """Squared Sampson distances (..., n) of the points under F (..., 3, 3)."""
    hk, hl = np.c_[xk, np.ones(len(xk))], np.c_[xl, np.ones(len(xl))]
    with np.errstate(all="ignore"):
        Fx, Ftx = np.einsum("...ij,nj->...ni", F, hk), np.einsum("...ji,nj->...ni", F, hl)
        r = (hl * Fx).sum(axis=-1)
        return r * r / (Fx[..., 0] ** 2 + Fx[..., 1] ** 2 + Ftx[..., 0] ** 2 + Ftx[..., 1] ** 2)


def epipolar_rows(a, b):
    one = np.ones(len(a))
    return np.stack([b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0], b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1], a[:, 0], a[:, 1], one], axis=1)


def finish(f, Tk, Tl):
    """F^ (9,) in normalised units -> rank 2, denormalised, |F| = 1, largest entry positive (the host step of the library)."""
    U, s, Vt = np.linalg.svd(f.reshape(3, 3))
    F = Tl.T @ (U @ np.diag([s[0], s[1], 0.0]) @ Vt) @ Tk
    F = F / np.linalg.norm(F)
    return -F if F.flat[np.argmax(np.abs(F))] < 0 else F


def _setup(xk, xl):
    """(T_k, T_l, normalised epipolar rows (n, 9)) of a pair's shared observations."""
    ck, sk = ref.hartley(xk)
    cl, sl = ref.hartley(xl)
    return T.hartley_T(ck, sk), T.hartley_T(cl, sl), epipolar_rows(sk * (xk - ck), sl * (xl - cl))


def _hypotheses(rows, Tk, Tl, k, l, seed, hs, linear):
    """The hypotheses ``hs`` of pair (k, l): F (len(hs), 3, 3) and F^ (len(hs), 9), NaN where degenerate, and the pivots."""
    n = len(rows)
    Fh, fh, pivot = np.full((len(hs), 3, 3), np.nan), np.full((len(hs), 9), np.nan), np.full(len(hs), np.nan)
    for i, h in enumerate(hs):
        r8 = rows[sample(seed, k, l, int(h), n)]
        if not np.isfinite(r8).all():
            continue
        if linear == "eigh":
            w, V = np.linalg.eigh(r8.T @ r8)
            f = V[:, 0]
        else:
            _, s, Vt = np.linalg.svd(r8, full_matrices=True)
            w, f = np.concatenate([s, [0.0]])[::-1] ** 2, Vt[8]
        pivot[i] = w[1] / w[8]
        Fd = Tl.T @ f.reshape(3, 3) @ Tk
        if w[1] > T.REL_PIVOT * w[8] and np.isfinite(Fd).all():
            Fh[i], fh[i] = Fd, f
    return Fh, fh, pivot


def hypothesis_counts(xk, xl, k, l, threshold, seed, hs, linear="eigh"):
    """(counts, margin, pivot) of the entries ``hs`` of the pair's count table alone (any h >= 0: a hypothesis depends on
    (seed, k, l, h) only), with the premise figures of robust_fundamental over those hypotheses."""
    out = np.full(len(hs), -1, np.int32)
    if len(xk) < 8:
        return out, np.inf, np.full(len(hs), np.nan)
    with np.errstate(all="ignore"):
        Tk, Tl, rows = _setup(xk, xl)
        Fh, _, pivot = _hypotheses(rows, Tk, Tl, k, l, seed, hs, linear)
        ok = np.isfinite(Fh).all(axis=(1, 2))
        d2, thr2 = sampson_d2(Fh, xk, xl), threshold * threshold
        margin = np.nanmin(np.abs(d2[ok] / thr2 - 1.0)) if ok.any() else np.inf
        return np.where(ok, (d2 <= thr2).sum(axis=1), -1).astype(np.int32), margin, pivot


def robust_fundamental(xk, xl, k, l, threshold, n_hyp, seed, n_refit, linear="eigh"):
    """One pair.  A dict: F (3, 3), quality (2,), status, n_inliers, best, mask (n,), hyp_count (H,), the figures of the
    parity premises: ``margin`` -- the smallest |d^2 / threshold^2 - 1| over every distance compared with the threshold --
    and ``pivot`` (H,) -- lambda_2 / lambda_max of each hypothesis --, and the trace of the refit loop: ``n_accepted`` -- the
    refits that were kept --, ``n_changed`` -- those of them whose inlier set differs from the one before -- and ``end`` --
    "rejected" (a refit's own inlier set was smaller), "solver" (a refit's eigen-problem failed), "exhausted" (all n_refit
    ran), or "" for a pair whose status is not 0."""
    n, H, thr2 = len(xk), int(n_hyp), threshold * threshold
    out = {"F": np.full((3, 3), np.nan), "quality": np.full(2, np.nan), "status": 1, "n_inliers": 0, "best": -1,
           "mask": np.zeros(n, bool), "hyp_count": np.full(H, -1, np.int32), "margin": np.inf, "pivot": np.full(H, np.nan),
           "n_accepted": 0, "n_changed": 0, "end": ""}
    if n < 8:
        return out
    with np.errstate(all="ignore"):
        Tk, Tl, rows = _setup(xk, xl)
        Fh, fh, out["pivot"] = _hypotheses(rows, Tk, Tl, k, l, seed, range(H), linear)
        ok = np.isfinite(Fh).all(axis=(1, 2))
        d2 = sampson_d2(Fh, xk, xl)  # (H, n)
        out["hyp_count"] = np.where(ok, (d2 <= thr2).sum(axis=1), -1).astype(np.int32)
        if ok.any():
            out["margin"] = np.nanmin(np.abs(d2[ok] / thr2 - 1.0))
    best = int(np.argmax(out["hyp_count"]))
    if out["hyp_count"][best] < 0:
        out["status"] = 2
        return out
    out["best"] = best
    if out["hyp_count"][best] < 8:
        out["status"] = 4
        return out
    mask, dd = d2[best] <= thr2, d2[best]
    F, ratio, end, n_acc, n_chg = finish(fh[best], Tk, Tl), 0.0, "exhausted", 0, 0
    for _ in range(n_refit):
        Fr, q, st = T.fundamental(xk[mask], xl[mask], linear)
        if st != 0:
            end = "solver"
            break
        dr = sampson_d2(Fr, xk, xl)
        out["margin"] = min(out["margin"], np.abs(dr / thr2 - 1.0).min())
        if (dr <= thr2).sum() < mask.sum():
            end = "rejected"
            break
        n_acc, n_chg = n_acc + 1, n_chg + int(not np.array_equal(dr <= thr2, mask))
        F, ratio, mask, dd = Fr, q[1], dr <= thr2, dr
    out.update(F=F, quality=np.array([np.sqrt(dd[mask].sum() / mask.sum()), ratio]), status=0, n_inliers=int(mask.sum()), mask=mask,
               n_accepted=n_acc, n_changed=n_chg, end=end)
    return out


def two_view_robust(pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hyp=512, seed=0, n_refit=2, linear="eigh"):
    """A dict of arrays over the pairs: F (P, 3, 3), quality (P, 2), n_shared, n_inliers, best, status (P,), inlier (P, N),
    hyp_count (P, H), margin (P,), pivot (P, H), and the refit trace n_accepted, n_changed, end (P,)."""
    pt_ptr, cam_idx, xy = T._list(pt_ptr, cam_idx, xy, n_images)
    pairs = np.asarray(pairs).reshape(-1, 2)
    N, res, ns = len(pt_ptr) - 1, [], []
    inl = np.zeros((len(pairs), N), bool)
    for i, (k, l) in enumerate(pairs):
        ids, xk, xl = T.shared(pt_ptr, cam_idx, xy, k, l)
        r = robust_fundamental(xk, xl, int(k), int(l), threshold, n_hyp, seed, n_refit, linear)
        inl[i, ids[r["mask"]]] = True
        res.append(r)
        ns.append(len(ids))
    out = {key: np.array([r[key] for r in res]) for key in ("F", "quality", "n_inliers", "best", "status", "hyp_count", "margin", "pivot",
                                                            "n_accepted", "n_changed", "end")}
    out.update(n_shared=np.array(ns, np.int64), inlier=inl)
    for v in out.values():
        v.setflags(write=False)
    return out


def relative_pose(pt_ptr, cam_idx, xy, K, pair, threshold, n_hyp=512, seed=0, n_refine=2, linear="eigh"):
    """(R, t, X, info) as lib.initialization.relative_pose with ``ransac_threshold``: the robust F, the inliers alone."""
    k, l = pair
    n = len(pt_ptr) - 1
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ids, xk, xl = T.shared(pt_ptr, cam_idx, xy, k, l)
    r = robust_fundamental(xk, xl, int(k), int(l), threshold, n_hyp, seed, 2, linear)
    inlier = np.zeros(n, bool)
    inlier[ids[r["mask"]]] = True
    info = {"n_front": np.zeros(4, np.int64), "status": int(r["status"]), "F": r["F"], "n_shared": len(ids), "inlier": inlier,
            "n_inliers": r["n_inliers"], "quality": np.full((n, 3), np.nan)}
    if r["status"] != 0:
        return (*T.no_pose(n), info)
    ids, xk, xl = ids[r["mask"]], xk[r["mask"]], xl[r["mask"]]
    return (*T.choose_candidate(K, pair, T.pose_candidates(K[l].T @ r["F"] @ K[k]), ids, xk, xl, info, n_refine)[:3], info)


def bootstrap(pt_ptr, cam_idx, xy, K, threshold, n_hyp=512, seed=0, linear="eigh", start_pair=None, min_points=12, max_rms=None):
    """(R, t, X, info) as lib.initialization.bootstrap with ``ransac_threshold``: the driver of tests/_bootstrap_ref.py with the
    robust relative_pose above as its start step, and tests/_twoview_ref.py's plain registration and triangulation."""
    R, t, X, info, _ = B.bootstrap(pt_ptr, cam_idx, xy, K, lambda pair: relative_pose(pt_ptr, cam_idx, xy, K, pair, threshold, n_hyp, seed, linear=linear),
                                   T.register_plain(pt_ptr, cam_idx, xy, K, min_points), T.triangulate_plain, start_pair, max_rms)
    return R, t, X, {key: info[key] for key in B.PLAIN_KEYS}
