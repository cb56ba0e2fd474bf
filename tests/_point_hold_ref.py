"""NumPy references of held points (include/mvba.h, mvba_set_point_hold), two independent statements of
"a held point has no unknowns":
  (a) dense, for small scenes: J = [J_X | J_C P] with the held points' columns deleted, H = 2 J^T J with its diagonal times
      (1 + c), the step -H^-1 (2 J^T e); and the covariance (J^T J)^-1 through a QR of J, as
      tests/_constraints_ref.py::dense_covariance_mapped takes it;
  (b) an engine: the oracle (with parameter maps, squared or robust loss) whose E_a^-1 is zero at held points, so that Y, b
      and dX are -- dressed in the HipEngine's protocol, so that the product's lm_loop and BundleAdjuster run over it.
Test infrastructure only."""
import numpy as np

from _engines import HostOracleEngine
from _constraints_ref import ConstrainedOracleEngine, ConstrainedRobustEngine, map_matrix
from lib.bundle_adjustment import BundleAdjuster
from oracle import ba_oracle as O


# ---------------------------------------------------------------- (a) dense
def _dense_jacobian(n, m, pt_ptr, cam_idx, xy, f0, col, n_free, held, X, f, u, t, R):
    """(e (2 n_obs,), J (2 n_obs, 3 n_free_points + n_free), free point indices, P)."""
    pt_ptr = np.asarray(pt_ptr, np.int64)
    cam = np.asarray(cam_idx, np.int64)
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    e, JX, JC = O.jacobians(X, f, u, t, R, f0, pt, cam, np.asarray(xy, np.float64).reshape(-1, 2))
    n_obs = len(cam)
    J = np.zeros((2 * n_obs, 3 * n + 9 * m))
    rows = np.arange(2 * n_obs).reshape(n_obs, 2)
    for c in range(3):
        J[rows, (3 * pt + c)[:, None]] = JX[:, :, c]
    for c in range(9):
        J[rows, (3 * n + 9 * cam + c)[:, None]] = JC[:, :, c]
    P = map_matrix(col, n_free)
    free = np.nonzero(~np.asarray(held, bool))[0]
    keep = (3 * free[:, None] + np.arange(3)).reshape(-1)
    return e.reshape(-1), np.concatenate([J[:, keep], J[:, 3 * n:] @ P], axis=1), free, P


def dense_step(n, m, pt_ptr, cam_idx, xy, f0, col, n_free, held, c, X, f, u, t, R):
    """One damped step of the problem without the held points' unknowns: {"dX" (n, 3), zeros where held, "dxi" (9 m,)}."""
    e, J, free, P = _dense_jacobian(n, m, pt_ptr, cam_idx, xy, f0, col, n_free, held, X, f, u, t, R)
    H = 2.0 * J.T @ J
    i = np.arange(H.shape[0])
    H[i, i] *= 1.0 + c
    step = -np.linalg.solve(H, 2.0 * J.T @ e) if H.shape[0] else np.zeros(0)
    dX = np.zeros((n, 3))
    dX[free] = step[:3 * len(free)].reshape(-1, 3)
    return {"dX": dX, "dxi": P @ step[3 * len(free):], "cond_H": np.linalg.cond(H) if H.shape[0] else 1.0}


def dense_covariance_held(n, m, pt_ptr, cam_idx, xy, f0, col, n_free, held, X, f, u, t, R):
    """Unit covariance of the same problem: point blocks (zeros where held), camera blocks, the joint camera covariance."""
    _, J, free, P = _dense_jacobian(n, m, pt_ptr, cam_idx, xy, f0, col, n_free, held, X, f, u, t, R)
    _, Rq = np.linalg.qr(J)
    Ri = np.linalg.inv(Rq)
    Cm = Ri @ Ri.T
    pts = np.zeros((n, 3, 3))
    for i, a in enumerate(free):
        pts[a] = Cm[3 * i:3 * i + 3, 3 * i:3 * i + 3]
    nf = 3 * len(free)
    full = P @ Cm[nf:, nf:] @ P.T
    cams = np.stack([full[9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(m)])
    return {"points": pts, "cameras": cams, "cameras_full": full}


# ---------------------------------------------------------------- (b) the engine
class _HoldMixin:
    """reduced_system with E_a^-1 = 0 at held points; without a mask (or an empty one) the engine below it, untouched."""
    _held = None
    n_held_points = 0

    def set_point_hold(self, mask):
        if mask is None:
            self._held, self.n_held_points = None, 0
            return
        mask = np.asarray(mask)
        assert mask.dtype == np.bool_ and mask.shape == (self.n,)
        self._held = mask.copy() if mask.any() else None
        self.n_held_points = int(mask.sum())

    def reduced_system(self, c):
        if self._held is None:
            return super().reduced_system(c)
        from scipy.sparse import bsr_matrix

        m = self.m
        Ec = self.E.copy()
        i3 = np.arange(3)
        Ec[:, i3, i3] *= 1.0 + c
        Ec[self._held] = np.eye(3)  # (never inverted: a held point seen once is legal)
        self.Einv = np.linalg.inv(Ec)
        self.Einv[self._held] = 0.0
        Y = np.einsum("oij,ojk->oik", self.Einv[self.pt], self.F)
        shape = (3 * self.n, 9 * m)
        Fs = bsr_matrix((self.F, self.cam, self.pt_ptr), shape=shape)
        Ys = bsr_matrix((Y, self.cam, self.pt_ptr), shape=shape)
        A = -np.asarray((Fs.T.tocsr() @ Ys.tocsr()).todense())
        b = O._segsum(self.cam, np.einsum("oji,oj->oi", Y, self.dP[self.pt]), m) - self.dF
        for k in range(m):
            Gk = self.G[k].copy()
            Gk[np.arange(9), np.arange(9)] *= 1.0 + c
            A[9 * k:9 * k + 9, 9 * k:9 * k + 9] += Gk
        return A, b.reshape(-1)


class HeldOracleEngine(_HoldMixin, ConstrainedOracleEngine):
    pass


class HeldRobustEngine(_HoldMixin, ConstrainedRobustEngine):
    """... and the device-log and similarity entry points the adjuster calls, as tests/_engines.py gives them to the squared one
    (optimize(is_debug=True) clears the log before it writes to it)."""
    snapshot, snapshot_count, snapshot_read = HostOracleEngine.snapshot, HostOracleEngine.snapshot_count, HostOracleEngine.snapshot_read
    snapshot_clear, apply_similarity = HostOracleEngine.snapshot_clear, HostOracleEngine.apply_similarity


class HeldRefAdjuster(BundleAdjuster):
    """The product's BundleAdjuster (normalisation, hold front end, LM loop, way back) over reference (b)."""

    def _make_engine(self, n_points, n_images, pt_ptr, cam_idx, xy, f0, axis, **kw):
        cls = HeldRobustEngine if kw else HeldOracleEngine
        return cls(n_points, n_images, pt_ptr, cam_idx, np.asarray(xy, np.float64).reshape(-1, 2), f0, axis, **kw)


def masks(n, seed=7):
    """The masks the one-step tests run under: name -> bool (n,).  "random40" goes with the map hold_intr."""
    one = np.zeros(n, bool)
    one[n // 2] = True
    third = np.arange(n) % 3 == 0
    but_one = np.ones(n, bool)
    but_one[n // 3] = False
    return {"one": one, "every_third": third, "all_but_one": but_one, "all": np.ones(n, bool),
            "random40": np.random.default_rng(seed).random(n) < 0.4}
