"""NumPy reference of the robust losses (include/mvba.h, mvba_create_robust): the oracle engine with the
cost sum rho(|e|^2) and IRLS-weighted linearisation -- every row of an observation (e, J_X, J_C) scaled by sqrt(w),
w = rho'(s) at the linearisation point.  The product's own lm_loop runs over it unchanged.  Test infrastructure only."""
import numpy as np

from oracle import ba_oracle as O

LOSSES = ("squared", "huber", "cauchy")


def rho(s, b, loss):
    s = np.asarray(s, np.float64)
    if loss == "huber":
        return np.where(s <= b, s, 2.0 * np.sqrt(b * s) - b)
    if loss == "cauchy":
        return b * np.log1p(s / b)
    return s


def weight(s, b, loss):
    s = np.asarray(s, np.float64)
    if loss == "huber":
        return np.where(s <= b, 1.0, np.sqrt(b / np.maximum(s, b)))
    if loss == "cauchy":
        return 1.0 / (1.0 + s / b)
    return np.ones_like(s)


def robust_cost(X, f, u, t, R, f0, pt, cam, xy, b, loss):
    e = O.residuals(X, f, u, t, R, f0, pt, cam, xy)
    return float(rho((e * e).sum(axis=1), b, loss).sum())


class RobustOracleEngine(O.OracleEngine):
    """OracleEngine with E = sum rho(|e|^2) and the rows of the normal equations weighted by w (J^T W J, J^T W e)."""

    def __init__(self, *a, loss="huber", loss_scale=1.0, **kw):
        super().__init__(*a, **kw)
        self.loss = loss
        self.loss_b = (float(loss_scale) / self.f0) ** 2

    def _cost_at(self, X, f, u, t, R):
        return robust_cost(X, f, u, t, R, self.f0, self.pt, self.cam, self.xy, self.loss_b, self.loss)

    def cost(self):
        return self._global_sum(self._cost_at(self.X, self.f, self.u, self.t, self.R))

    def linearize(self):
        e, JX, JC = O.jacobians(self.X, self.f, self.u, self.t, self.R, self.f0, self.pt, self.cam, self.xy)
        self.w = weight((e * e).sum(axis=1), self.loss_b, self.loss)
        sw = np.sqrt(self.w)
        e, JX, JC = e * sw[:, None], JX * sw[:, None, None], JC * sw[:, None, None]
        self.e, self.JX, self.JC = e, JX, JC
        self.dP = 2.0 * O._segsum(self.pt, np.einsum("ori,or->oi", JX, e), self.n)
        self.dF = 2.0 * O._segsum(self.cam, np.einsum("ori,or->oi", JC, e), self.m)
        self.E = 2.0 * O._segsum(self.pt, np.einsum("ori,orj->oij", JX, JX), self.n)
        self.F = 2.0 * np.einsum("ori,orj->oij", JX, JC)
        self.G = 2.0 * O._segsum(self.cam, np.einsum("ori,orj->oij", JC, JC), self.m)

    def apply_step(self, dxi):
        super().apply_step(dxi)
        return self._cost_at(self.tX, self.tf, self.tu, self.tt, self.tR)


def inject_outliers(xy, frac, lo, hi, seed=0):
    """A copy of ``xy`` (n_obs, 2) with ``frac`` of the observations displaced by lo..hi pixels in a random direction;
    returns (xy, mask of the displaced ones)."""
    rng = np.random.default_rng(seed)
    xy = np.array(xy, np.float64, copy=True).reshape(-1, 2)
    n = xy.shape[0]
    idx = rng.choice(n, size=max(1, int(round(frac * n))), replace=False)
    ang = rng.uniform(0.0, 2.0 * np.pi, idx.size)
    r = rng.uniform(lo, hi, idx.size)
    xy[idx] += np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    mask = np.zeros(n, bool)
    mask[idx] = True
    return xy, mask
