"""The host driver of the incremental reconstruction that the references of tests/_*_ref.py share: the control flow of
lib/initialization.py's bootstrap written once, with its three steps passed in as plain callables --

    start(pair) -> (R2 (2, 3, 3), t2 (2, 3), X (N, 3), info)              the relative pose of a pair and the points it gives
    register(X, point_ok, camera_ok) -> None | (c, R_c, t_c, sel, dropped)  the next camera, its pose, the (n_obs,) mask of the
                                                                            observations it was registered from and of those it
                                                                            drops for good (None: the step verifies nothing)
    triangulate(K, R, t, ptr, cam, xy) -> (X, quality, status, used, extras)  the points of a round; ``used``: which observations
                                                                            of the list, ``extras``: a dict kept for the caller

-- so that a reference states only what its option changes.  It imports nothing from the library.  Test infrastructure only."""
import numpy as np

PLAIN_KEYS = ("axis", "camera_ok", "point_ok", "order", "start_pair")  # the info of the library without a threshold,
ROBUST_KEYS = PLAIN_KEYS + ("obs_ok", "inlier")  # and with a robust registration


def most_inliers(ri, todo, cam_idx, usable, min_points):
    """What a robust registration takes out of its result ``ri`` over the cameras ``todo``: None, or (i, c, sel, dropped) of the
    camera with the most inliers among those of status 0 with at least ``min_points`` (the lowest index on ties): its position
    in ``todo``, its index, its inlier observations and its ``usable`` observations that are not inliers."""
    cand = np.nonzero((ri["status"] == 0) & (ri["n_inliers"] >= min_points))[0]
    if len(cand) == 0:
        return None
    i = int(cand[np.argmax(ri["n_inliers"][cand])])
    c = int(todo[i])
    sel = ri["inlier"] & (cam_idx == c)
    return i, c, sel, (cam_idx == c) & usable & ~sel


def bootstrap(pt_ptr, cam_idx, xy, K, start, register, triangulate, start_pair=None, max_rms=None):
    """(R, t, X, info, trace) as lib.initialization.bootstrap, on the host; ``K`` (m, 3, 3) projects to the units of xy.  ``info``:
    axis, camera_ok, point_ok, obs_ok, inlier, tri_inlier, order, start_pair; ``trace``: ``start`` -- what the start step returned
    for the pair taken --, ``extras`` -- those of every round's triangulation -- and ``frame`` -- (R0, t0, s) of the output frame:
    X_out = (X - t0) R0 / s."""
    pt_ptr, cam_idx, xy = np.asarray(pt_ptr), np.asarray(cam_idx), np.asarray(xy, np.float64).reshape(-1, 2)
    m, n = len(K), len(pt_ptr) - 1
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    if start_pair is None:  # the 16 most co-visible pairs with at least 8 shared points
        vis = np.zeros((n, m), np.int64)
        vis[pt, cam_idx] = 1
        count = vis.T @ vis
        ks, ls = np.triu_indices(m, 1)
        tried = [(int(ks[i]), int(ls[i])) for i in np.argsort(-count[ks, ls], kind="stable") if count[ks[i], ls[i]] >= 8][:16]
    else:
        tried = [tuple(start_pair)]
    best = None
    for pair in tried:  # the largest median ray angle among those of status 0
        out = start(pair)
        if out[3]["status"] == 0:
            angle = float(np.nanmedian(out[3]["quality"][:, 2]))
            if best is None or angle > best[0]:
                best = (angle, pair, out)
    if best is None:
        raise ValueError("no start pair")
    _, pair, first = best
    X = first[2]
    R, t = np.full((m, 3, 3), np.nan), np.full((m, 3), np.nan)
    R[list(pair)], t[list(pair)] = first[0], first[1]
    camera_ok = np.zeros(m, bool)
    camera_ok[list(pair)] = True
    point_ok = np.isfinite(X).all(axis=1)
    order, extras = list(pair), []
    obs_ok, inlier = np.ones(len(cam_idx), bool), np.zeros(len(cam_idx), bool)
    tri_inlier = point_ok[pt] & camera_ok[cam_idx]
    while not camera_ok.all():
        reg = register(X, point_ok, camera_ok)
        if reg is None:
            break
        c, R[c], t[c], sel, dropped = reg
        if dropped is not None:
            obs_ok &= ~dropped
            inlier |= sel
        camera_ok[c] = True
        order.append(c)
        keep = obs_ok & camera_ok[cam_idx]  # the list of the registered cameras without what was dropped, cameras renumbered
        ptr = np.concatenate([[0], np.cumsum(np.bincount(pt[keep], minlength=n))]).astype(np.int64)
        ids = np.nonzero(camera_ok)[0]
        X, q, s, used, ex = triangulate(K[ids], R[ids], t[ids], ptr, (np.cumsum(camera_ok) - 1)[cam_idx[keep]].astype(np.int32), xy[keep])
        extras.append(ex)
        point_ok = (s == 0) & (q[:, 1] > 0)
        if max_rms is not None:
            point_ok &= q[:, 0] <= max_rms
        X[~point_ok] = np.nan
        tri_inlier = np.zeros(len(cam_idx), bool)
        tri_inlier[np.nonzero(keep)[0]] = used
        tri_inlier &= point_ok[pt]
    for c in (0, 1):
        if not camera_ok[c]:
            raise ValueError(f"camera {c} could not be registered")
    R0, t0, s = R[0].copy(), t[0].copy(), np.linalg.norm(t[1] - t[0])
    X, R, t = ((X - t0) @ R0) / s, R0.T @ R, ((t - t0) @ R0) / s
    axis = "x-right_z-forward" if abs(t[1, 0]) >= abs(t[1, 1]) else "x-up_z-forward"
    info = {"axis": axis, "camera_ok": camera_ok, "point_ok": point_ok, "obs_ok": obs_ok, "inlier": inlier, "tri_inlier": tri_inlier,
            "order": order, "start_pair": pair}
    return R, t, X, info, {"start": first, "extras": extras, "frame": (R0, t0, s)}
