"""NumPy reference of parameter maps (include/mvba.h, mvba_set_parameter_map): the oracle engine whose
dense solve is that of the re-parameterised problem,  (P^T A P) x = P^T b,  dxi = P x,  with P[g][col g] = 1 -- dressed
in the HipEngine's protocol so that the product's lm_loop and BundleAdjuster run over it -- and the dense covariance
under a map.  Test infrastructure only."""
import numpy as np

from _engines import HostOracleEngine
from _robust_ref import RobustOracleEngine
from lib.bundle_adjustment import BundleAdjuster
from oracle import ba_oracle as O


def map_matrix(col, n_free):
    """P (len(col), n_free), 0/1."""
    col = np.asarray(col)
    P = np.zeros((col.size, int(n_free)))
    g = np.nonzero(col >= 0)[0]
    P[g, col[g]] = 1.0
    return P


class _MapMixin:
    """solve_reduced through a parameter map; without one (or after None) the oracle's own."""
    _P = None

    def set_parameter_map(self, col, n_free=None):
        if col is None:
            self._P = None
            self.n_free = 9 * self.m - 7
            return
        col = np.asarray(col, np.int64).reshape(-1)
        assert col.shape == (9 * self.m,)
        n_free = int(col.max()) + 1 if n_free is None else int(n_free)
        assert (col[self.removed] == -1).all()
        self._P = map_matrix(col, n_free)
        self.map_col, self.n_free = col, n_free

    def solve_reduced(self, A, b):
        if self._P is None:
            return super().solve_reduced(A, b)
        P = self._P
        self.n_solves += 1
        if P.shape[1] == 0:
            self.dxi_red = np.zeros(0)
            return np.zeros(9 * self.m)
        self.A, self.b = P.T @ A @ P, P.T @ b
        self.dxi_red = np.linalg.solve(self.A, self.b)
        return P @ self.dxi_red


class ConstrainedOracleEngine(_MapMixin, HostOracleEngine):
    pass


class ConstrainedRobustEngine(_MapMixin, RobustOracleEngine):
    pass


class RefAdjuster(BundleAdjuster):
    """The product's BundleAdjuster (normalisation, map front end, LM loop, way back) over the reference engine."""

    def _make_engine(self, n_points, n_images, pt_ptr, cam_idx, xy, f0, axis, **kw):
        return ConstrainedOracleEngine(n_points, n_images, pt_ptr, cam_idx, np.asarray(xy, np.float64).reshape(-1, 2), f0, axis)


def dense_covariance_mapped(n, m, pt_ptr, cam_idx, xy, f0, col, n_free, X, f, u, t, R):
    """Unit covariance of the re-parameterised problem, built as tests/_covariance_ref.py::dense_covariance builds the
    default one: J = [J_X | J_C P], (J^T J)^-1 through a QR of J, expanded by blockdiag(I, P)."""
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
    P = map_matrix(col, n_free)
    Jm = np.concatenate([J[:, :3 * n], J[:, 3 * n:] @ P], axis=1)
    _, Rq = np.linalg.qr(Jm)
    Ri = np.linalg.inv(Rq)
    Cm = Ri @ Ri.T
    pts = np.stack([Cm[3 * a:3 * a + 3, 3 * a:3 * a + 3] for a in range(n)]) if n else np.zeros((0, 3, 3))
    full = P @ Cm[3 * n:, 3 * n:] @ P.T
    cams = np.stack([full[9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(m)])
    return {"points": pts, "cameras": cams, "cameras_full": full, "sigma_reduced": Cm[3 * n:, 3 * n:]}
