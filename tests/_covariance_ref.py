"""NumPy references for the marginal covariances (mvba_covariance) -- test infrastructure only.

Unit covariance C = (J^T J)^-1 over the free parameters (all 3N + 9m minus oracle.ba_oracle.gauge_removed), zero rows and
columns at the gauge parameters; J is the Jacobian of oracle.ba_oracle.jacobians (units x / f0).
  dense_covariance   J itself, gauge columns dropped, inv(J^T J) through a QR of J: small scenes only
  schur_covariance   the oracle's undamped reduced system S (H = 2 J^T J): cameras 2 S^-1, points
                     C_a = 2 [E_a^-1 + E_a^-1 (sum_{k,l in obs(a)} F_ak Sigma_kl F_al^T) E_a^-1],  Sigma = S^-1 expanded
"""
import numpy as np

from oracle import ba_oracle as O


def dense_covariance(n, m, pt_ptr, cam_idx, xy, f0, axis, X, f, u, t, R):
    pt_ptr = np.asarray(pt_ptr, np.int64)
    cam = np.asarray(cam_idx, np.int64)
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    _, JX, JC = O.jacobians(X, f, u, t, R, f0, pt, cam, np.asarray(xy, np.float64).reshape(-1, 2))
    n_obs = len(cam)
    J = np.zeros((2 * n_obs, 3 * n + 9 * m))
    rows = np.arange(2 * n_obs).reshape(n_obs, 2)
    for c in range(3):
        J[rows, (3 * pt + c)[:, None]] = JX[:, :, c]
    for c in range(9):
        J[rows, (3 * n + 9 * cam + c)[:, None]] = JC[:, :, c]
    keep = np.setdiff1d(np.arange(3 * n + 9 * m), 3 * n + O.gauge_removed(axis))
    # (J^T J)^-1 = R^-1 R^-T from J = Q R: J^T J is never formed, so its condition number (cond(J)^2, 5e11 on the 60 x 7
    # golden scene) does not enter the reference
    _, Rq = np.linalg.qr(J[:, keep])
    Ri = np.linalg.inv(Rq)
    C = np.zeros((3 * n + 9 * m,) * 2)
    C[np.ix_(keep, keep)] = Ri @ Ri.T
    pts = np.stack([C[3 * a:3 * a + 3, 3 * a:3 * a + 3] for a in range(n)]) if n else np.zeros((0, 3, 3))
    full = C[3 * n:, 3 * n:]
    cams = np.stack([full[9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(m)])
    return {"points": pts, "cameras": cams, "cameras_full": full}


def schur_sigma(engine):
    """Sigma = S^-1 (9m x 9m, zeros at the gauge slots) of a linearised OracleEngine, undamped."""
    A, _ = engine.reduced_system(0.0)
    keep = engine.keep
    S = np.zeros_like(A)
    S[np.ix_(keep, keep)] = np.linalg.inv(A[np.ix_(keep, keep)])
    return S


def point_blocks(E, F, pt_ptr, cam_idx, sigma, points=None):
    """C_a of the point formula for the points `points` (default all): E (N,3,3) and F (n_obs,3,9) undamped as the
    oracle forms them, sigma (9m, 9m) = S^-1."""
    pt_ptr = np.asarray(pt_ptr, np.int64)
    cam = np.asarray(cam_idx, np.int64)
    m = sigma.shape[0] // 9
    S4 = sigma.reshape(m, 9, m, 9)
    idx = range(len(pt_ptr) - 1) if points is None else points
    out = []
    for a in idx:
        o0, o1 = pt_ptr[a], pt_ptr[a + 1]
        Fa, ka = F[o0:o1], cam[o0:o1]
        blocks = S4[ka][:, :, ka].transpose(0, 2, 1, 3)  # (d, d, 9, 9): Sigma_{k_o k_o'}
        Q = np.einsum("oij,opjk,plk->il", Fa, blocks, Fa)
        Ei = np.linalg.inv(E[a])
        out.append(2.0 * (Ei + Ei @ Q @ Ei))
    return np.stack(out) if out else np.zeros((0, 3, 3))


def schur_covariance(n, m, pt_ptr, cam_idx, xy, f0, axis, X, f, u, t, R, points=None):
    g = O.OracleEngine(n, m, pt_ptr, cam_idx, xy, f0, axis)
    g.set_params(X, f, u, t, R)
    g.linearize()
    sigma = schur_sigma(g)
    full = 2.0 * sigma
    cams = np.stack([full[9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(m)])
    return {"points": point_blocks(g.E, g.F, pt_ptr, cam_idx, sigma, points), "cameras": cams, "cameras_full": full}


# ---- the same two constructions in extended precision (np.longdouble), for the checks where double rounding of the normal
# equations, not the formulas, decides the agreement (cond(J^T J) = 5e11 on the 60 x 7 golden scene)
def _gj_inverse(A):
    """Gauss-Jordan inverse with partial pivoting in A's dtype (numpy.linalg has no long double)."""
    n = A.shape[0]
    M = np.concatenate([A, np.eye(n, dtype=A.dtype)], axis=1)
    rows = np.arange(n)
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        M[[c, p]] = M[[p, c]]
        M[c] /= M[c, c]
        M -= np.outer(np.where(rows == c, 0, M[:, c]), M[c])
    return M[:, n:]


def _jacobian_ld(n, m, pt_ptr, cam_idx, xy, f0, X, f, u, t, R):
    pt_ptr = np.asarray(pt_ptr, np.int64)
    cam = np.asarray(cam_idx, np.int64)
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    _, JX, JC = O.jacobians(X, f, u, t, R, f0, pt, cam, np.asarray(xy, np.float64).reshape(-1, 2))
    return pt, cam, JX.astype(np.longdouble), JC.astype(np.longdouble)


def dense_covariance_extended(n, m, pt_ptr, cam_idx, xy, f0, axis, X, f, u, t, R):
    """inv(J^T J) in long double (J itself as the oracle computes it, in double)."""
    pt, cam, JX, JC = _jacobian_ld(n, m, pt_ptr, cam_idx, xy, f0, X, f, u, t, R)
    n_obs = len(cam)
    J = np.zeros((2 * n_obs, 3 * n + 9 * m), np.longdouble)
    rows = np.arange(2 * n_obs).reshape(n_obs, 2)
    for c in range(3):
        J[rows, (3 * pt + c)[:, None]] = JX[:, :, c]
    for c in range(9):
        J[rows, (3 * n + 9 * cam + c)[:, None]] = JC[:, :, c]
    keep = np.setdiff1d(np.arange(3 * n + 9 * m), 3 * n + O.gauge_removed(axis))
    Jk = J[:, keep]
    C = np.zeros((3 * n + 9 * m,) * 2, np.longdouble)
    C[np.ix_(keep, keep)] = _gj_inverse(Jk.T @ Jk)
    return {"points": np.stack([C[3 * a:3 * a + 3, 3 * a:3 * a + 3] for a in range(n)]), "cameras_full": C[3 * n:, 3 * n:]}


def schur_covariance_extended(n, m, pt_ptr, cam_idx, xy, f0, axis, X, f, u, t, R):
    """The Schur construction of schur_covariance on the unit normal equations (E = Jx^T Jx, F = Jx^T Jc, G = sum Jc^T Jc:
    the factors 2 of H cancel) in long double."""
    pt, cam, JX, JC = _jacobian_ld(n, m, pt_ptr, cam_idx, xy, f0, X, f, u, t, R)
    E = np.zeros((n, 3, 3), np.longdouble)
    np.add.at(E, pt, np.einsum("ori,orj->oij", JX, JX))
    F = np.einsum("ori,orj->oij", JX, JC)
    Ei = np.stack([_gj_inverse(e) for e in E])
    S = np.zeros((9 * m, 9 * m), np.longdouble)
    for o in range(len(cam)):
        k = cam[o]
        S[9 * k:9 * k + 9, 9 * k:9 * k + 9] += JC[o].T @ JC[o]
    pt_ptr = np.asarray(pt_ptr, np.int64)
    for a in range(n):
        obs = range(pt_ptr[a], pt_ptr[a + 1])
        for o in obs:
            for p in obs:
                k, l = cam[o], cam[p]
                S[9 * k:9 * k + 9, 9 * l:9 * l + 9] -= F[o].T @ Ei[a] @ F[p]
    keep = np.setdiff1d(np.arange(9 * m), O.gauge_removed(axis))
    sig = np.zeros_like(S)
    sig[np.ix_(keep, keep)] = _gj_inverse(S[np.ix_(keep, keep)])
    S4 = sig.reshape(m, 9, m, 9)
    pts = []
    for a in range(n):
        o0, o1 = pt_ptr[a], pt_ptr[a + 1]
        ka = cam[o0:o1]
        Q = np.einsum("oij,opjk,plk->il", F[o0:o1], S4[ka][:, :, ka].transpose(0, 2, 1, 3), F[o0:o1])
        pts.append(Ei[a] + Ei[a] @ Q @ Ei[a])
    return {"points": np.stack(pts), "cameras_full": sig}
