"""Bundle adjustment with the call surface of the reference's
``lib/bundle_adjustment.py`` (class ``BundleAdjuster``: constructor :11-21,
``optimize`` :77-83/:202, ``get_log`` :204-206) on the MI355X engine.

What stays in Python, exactly as the reference does it:
  * the scene normalisation / de-normalisation with its sign quirk (:208-258),
  * ``f <- K[:,0,0]``, ``u <- K[:,:2,2]`` (K[1,1], K[2,2] ignored, :45-48),
  * the Levenberg-Marquardt control flow: c0 = 1e-4, reject iff ``E_ > E``
    (strict), ``c *= s`` / ``c /= s``, stop on ``|dE| <= tol`` or ``max_iter``,
    the per-iteration print and the debug log (:100-195).
Everything numerical per observation / point / reduced system runs in
``libmvba.so`` (hand-written HIP, see csrc/mvba.hip and its kernel headers csrc/mvba_*.h) through ``_mvba.HipEngine``.
There is no CPU fallback.
"""
from __future__ import annotations

import os
from typing import Any

import numpy as np
import numpy.typing as npt

from ._mvba import check_loss

AXES = {"x-right_z-forward": 0, "x-up_z-forward": 1}


def dense_to_observations(x: npt.NDArray, visibility_index: npt.NDArray | None):
    """Dense ``x (N,m,2)`` + bool mask (ref :37, :56-60) -> CSR-by-point list (pt_ptr, cam_idx, xy (n_obs, 2)).
    Invisible entries are dropped instead of multiplied by 0.  Without a mask, an ``x`` that is the
    transposed view of a stack of image arrays comes back as that stack, xy (m, N, 2): see below."""
    n, m = x.shape[:2]
    if visibility_index is None:  # everything visible: the list is the array itself (np.nonzero + a gather took 0.24 s at 1 M x 12)
        x = np.asarray(x, dtype=np.float64)
        planes = x.transpose(1, 0, 2)
        if not x.flags.c_contiguous and planes.flags.c_contiguous:
            # the reference caller's np.stack(x_list).transpose(1, 0, 2) (euclidiean_reconstruction.py:50): the memory is the m image
            # planes.  They go to the engine as they are -- xy of shape (m, N, 2), mvba_problem.xy_layout 1 -- and the device puts
            # them into observation order (the strided host copy below: 0.10 s at 1 M x 12, a third of the whole pipeline)
            xy = planes
        else:
            xy = np.ascontiguousarray(x.reshape(n * m, 2))
        cam_idx = np.empty((n, m), dtype=np.int32)
        cam_idx[:] = np.arange(m, dtype=np.int32)  # (a broadcast store: np.tile of the same 12 M entries took 0.07 s)
        return np.arange(0, (n + 1) * m, m, dtype=np.int64), cam_idx.reshape(-1), xy
    vis = np.asarray(visibility_index, dtype=np.bool_)
    pt, cam = np.nonzero(vis)
    pt_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(vis.sum(axis=1), out=pt_ptr[1:])
    xy = np.ascontiguousarray(np.asarray(x)[pt, cam], dtype=np.float64)
    return pt_ptr, cam.astype(np.int32), xy


def to_gauge_frame(X, R, t, axis: str):
    """Scene -> the frame BA works in (ref :208-240): camera 0 at the origin with identity pose,
    camera 1's baseline component along the gauge axis of unit size.  The divisor keeps the
    reference's quirk: its SIGN comes from the world-frame component of t1 - t0, its
    MAGNITUDE from the camera-0-frame component."""
    if axis not in AXES:
        raise ValueError()
    g = AXES[axis]  # 0: x-right (index 0), 1: x-up (index 1)
    R0 = R[0]
    dX, dt = X - t[0], t - t[0]
    s = np.sign(dt[1, g]) * (R0[:, g] @ dt[1])
    s = np.array([s])  # shape (1,), as the reference's
    return (dX @ R0) / s, R0.T @ R, (dt @ R0) / s


def from_gauge_frame(camera0: dict[str, Any], X, R, t):
    """The way back (ref :242-258): scale by |baseline| (an abs, :23-26), rotate by camera 0's
    original pose, shift by its original centre."""
    R0, t0, length = camera0["R"], camera0["t"], camera0["c0c1_len"]
    return t0 + (length * X) @ R0.T, R0 @ R, t0 + (length * t) @ R0.T


def from_gauge_frame_inverse(camera0: dict[str, Any], X, R, t):
    """The exact inverse of ``from_gauge_frame``: the input frame back into the gauge frame BA works in."""
    R0, t0, length = camera0["R"], camera0["t"], camera0["c0c1_len"]
    return ((X - t0) @ R0) / length, R0.T @ R, ((t - t0) @ R0) / length


def camera_frame_map(camera0: dict[str, Any]):
    """T (9, 9): how one camera's parameter increments (f, u, v, t, omega) map from the gauge frame to the input frame.
    f, u, v stay; t_in = t0 + L R0 t gives L R0; R_in = R0 R and R <- Rod(omega) R give omega_in = R0 omega."""
    R0, length = np.asarray(camera0["R"], dtype=np.float64), float(camera0["c0c1_len"])
    T = np.zeros((9, 9))
    T[:3, :3] = np.eye(3)
    T[3:6, 3:6] = length * R0
    T[6:9, 6:9] = R0
    return T


def covariance_to_input_frame(camera0: dict[str, Any], points=None, cameras=None, cameras_full=None):
    """Gauge-frame covariances -> the input frame: L^2 R0 C_a R0^T per point (N, 3, 3), T C_k T^T per camera (m, 9, 9),
    and blockdiag(T) C blockdiag(T)^T for the joint (9m, 9m) camera covariance.  Returns the three (None stays None)."""
    R0, length = np.asarray(camera0["R"], dtype=np.float64), float(camera0["c0c1_len"])
    T = camera_frame_map(camera0)
    P = None if points is None else length ** 2 * np.einsum("ij,ajk,lk->ail", R0, points, R0)
    Cc = None if cameras is None else np.einsum("ij,kjl,ml->kim", T, cameras, T)
    Cf = None
    if cameras_full is not None:
        m = cameras_full.shape[0] // 9
        Cf = np.einsum("ij,kjlm,nm->kiln", T, cameras_full.reshape(m, 9, m, 9), T).reshape(9 * m, 9 * m)
    return P, Cc, Cf


def residual_variance(E: float, n_obs: int, n_points: int, n_images: int, n_free: int | None = None, n_held: int = 0) -> float:
    """sigma^2 = E / (2 n_obs - (3 N + 9 m - 7)): the residual variance per image coordinate (units x / f0) at the
    solution; ValueError when the problem has no redundancy.  ``n_free``: the number of free camera unknowns under a
    parameter map (``parameter_map``), in the place of 9 m - 7.  ``n_held``: the number of held points (``hold_points``),
    which are not unknowns: 3 (N - n_held) in the place of 3 N."""
    n_pts = int(n_points) - int(n_held)
    if n_free is None:
        dof = 2 * int(n_obs) - (3 * n_pts + 9 * int(n_images) - 7)
        if dof <= 0:
            raise ValueError(f"no redundancy: 2 n_obs - (3 N + 9 m - 7) = {dof}")
        return float(E) / dof
    dof = 2 * int(n_obs) - (3 * n_pts + int(n_free))
    if dof <= 0:
        raise ValueError(f"no redundancy: 2 n_obs - (3 N + n_free) = {dof}")
    return float(E) / dof


# ---- parameter maps: which camera parameters are adjusted -------------------------------------
# slots of one camera, in the engine's order: f | u, v | t | omega
HOLD_NAMES = {"f": (0,), "u": (1, 2), "t": (3, 4, 5), "R": (6, 7, 8), "intrinsics": (0, 1, 2), "pose": (3, 4, 5, 6, 7, 8),
              "cameras": tuple(range(9))}
SHARE_NAMES = {"f": (0,), "u": (1, 2), "intrinsics": (0, 1, 2)}
SLOT_LABELS = ("f", "u", "v", "t_x", "t_y", "t_z", "omega_x", "omega_y", "omega_z")


def gauge_slots(axis: str):
    """The seven slots 9 k + p the gauge fixes: camera 0's t and omega, one component of camera 1's t."""
    if axis not in AXES:
        raise ValueError(f"axis must be one of {sorted(AXES)}, got {axis!r}")
    return np.array([3, 4, 5, 6, 7, 8, 12 + AXES[axis]])


def _slot_names(arg, table, what):
    names = [arg] if isinstance(arg, str) else list(arg)
    slots: set[int] = set()
    for nm in names:
        if not isinstance(nm, str) or nm not in table:
            raise ValueError(f"{what}: unknown name {nm!r} (known: {sorted(table)})")
        slots.update(table[nm])
    return slots


def parameter_map(n_images: int, axis: str = "x-right_z-forward", hold=None, share=None, share_groups=None):
    """(col, n_free) for ``HipEngine.set_parameter_map`` / ``mvba_set_parameter_map``: col (9 m,) int32, slot 9 k + p
    (p: f, u, v, t_x, t_y, t_z, omega_x, omega_y, omega_z) -> reduced unknown, -1 where held.

    ``hold``: names applied to every camera -- "f", "u" (both principal-point coordinates), "t", "R", "intrinsics"
    (f, u), "pose" (t, R), "cameras" (everything) -- one or several, or a bool array (m, 9), True = held.  The seven
    gauge slots are always held.  ``share``: names among "f", "u", "intrinsics": that parameter is ONE unknown for all
    cameras of a group.  ``share_groups``: int array (m,), equal labels form a group (default: one group of all
    cameras).  Order of the unknowns: the untied ones first, by ascending slot; the tied ones last, by (group label, p).
    A pose is held in the gauge frame BA works in (relative to camera 0 and the camera-0/1 baseline).
    ValueError: an unknown name, a slot both held by name and shared, a group some of whose members are held in a shared
    slot and some not."""
    m = int(n_images)
    gauge = gauge_slots(axis)
    held = np.zeros((m, 9), dtype=bool)
    held_by_name: set[int] = set()
    if hold is not None:
        if isinstance(hold, str) or (len(hold) and all(isinstance(v, str) for v in hold)):
            held_by_name = _slot_names(hold, HOLD_NAMES, "hold")
            held[:, sorted(held_by_name)] = True
        else:
            mask = np.asarray(hold)
            if mask.dtype != np.bool_ or mask.shape != (m, 9):
                raise ValueError(f"hold: names or a bool array of shape ({m}, 9), got {mask.dtype} {mask.shape}")
            held |= mask
    shared = _slot_names(share, SHARE_NAMES, "share") if share is not None else set()
    both = sorted(shared & held_by_name)
    if both:
        raise ValueError(f"slot {SLOT_LABELS[both[0]]!r} is both held and shared")
    if share_groups is None:
        labels = np.zeros(m, dtype=np.int64)
    else:
        labels = np.asarray(share_groups)
        if labels.shape != (m,) or labels.dtype.kind not in "iu":
            raise ValueError(f"share_groups: an int array of shape ({m},)")
    held_flat = held.reshape(-1).copy()
    held_flat[gauge[gauge < 9 * m]] = True  # (never in an intrinsic slot: sharing is not affected)
    col = np.full(9 * m, -1, dtype=np.int32)
    tied_sets = []  # (label, p, slots)
    tied_mask = np.zeros(9 * m, dtype=bool)
    for lab in np.unique(labels) if shared else ():
        cams = np.nonzero(labels == lab)[0]
        for p in sorted(shared):
            h = held[cams, p]
            if h.all():
                continue
            if h.any():
                raise ValueError(f"group {int(lab)}: slot {SLOT_LABELS[p]!r} is held for some of its cameras and shared by the others")
            if len(cams) > 1:  # (a group of one camera has nothing to tie: an ordinary unknown)
                tied_sets.append((lab, p, 9 * cams + p))
                tied_mask[9 * cams + p] = True
    free = np.nonzero(~held_flat & ~tied_mask)[0]
    col[free] = np.arange(len(free), dtype=np.int32)
    for i, (_, _, slots) in enumerate(tied_sets):
        col[slots] = len(free) + i
    return col, len(free) + len(tied_sets)


def point_hold_mask(n_points: int, hold_points, init_X=None):
    """``hold_points`` of ``BundleAdjuster`` as a bool mask (n_points,): a bool array (n_points,), True = held, or an integer
    array of point indices (any order, duplicates allowed).  With ``init_X`` (n_points, 3): its held rows must be finite.
    ValueError, the offending number in the message, for another dtype or shape, an index outside 0 .. n_points - 1, a held
    row that is not finite."""
    n = int(n_points)
    hp = np.asarray(hold_points)
    if hp.dtype == np.bool_:
        if hp.shape != (n,):
            raise ValueError(f"hold_points: a bool array must have shape ({n},), got {hp.shape}")
        mask = hp.copy()
    elif hp.dtype.kind in "iu" and hp.ndim == 1:
        bad = np.nonzero((hp < 0) | (hp >= n))[0]
        if len(bad):
            raise ValueError(f"hold_points: index {int(hp[bad[0]])} (entry {int(bad[0])}) is outside 0 .. {n - 1}")
        mask = np.zeros(n, dtype=bool)
        mask[hp] = True
    else:
        raise ValueError(f"hold_points: a bool array of shape ({n},) or a 1-d integer array of point indices, got {hp.dtype} {hp.shape}")
    if init_X is not None:
        X = np.asarray(init_X, dtype=np.float64)
        bad = np.nonzero(mask & ~np.isfinite(X).all(axis=1))[0]
        if len(bad):
            raise ValueError(f"hold_points: held point {int(bad[0])} starts from a position that is not finite ({len(bad)} such points)")
    return mask


def intrinsics_from(f, u, f0: float):
    """K_k = [[f,0,u0],[0,f,v0],[0,0,f0]] (ref :283-289): K[2,2] is forced to f0."""
    m = len(f)
    K = np.zeros((m, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, 0, 2], K[:, 1, 2] = u[:, 0], u[:, 1]
    K[:, 2, 2] = f0
    return K



class LevenbergMarquardt:
    """The reference's LM control state (:85-101, :118-195) over an engine that
    offers cost / linearize / try_step / commit; ``iterate()`` is one outer
    iteration: linearise once, retry with ``c *= s`` while the trial cost is
    strictly larger, commit."""

    def __init__(self, engine, scale_factor):
        self.engine, self.scale_factor = engine, scale_factor
        self.E = engine.cost()
        self.c = 0.0001
        self.count = 0

    def iterate(self):
        g = self.engine
        g.linearize()
        while True:  # no iteration cap, as the reference
            E_ = g.try_step(self.c)
            if E_ > self.E:
                self.c *= self.scale_factor
            else:
                break
        g.commit()
        self.count += 1
        delta = np.abs(E_ - self.E)
        return E_, delta

    def carry_on(self, E_):
        """ref :194-195"""
        self.E = E_
        self.c /= self.scale_factor


def lm_loop(engine, scale_factor, delta_tol, max_iter, on_state=None, verbose=True):
    """The reference's outer loop (:102-195).  Returns the final cost."""
    lm = LevenbergMarquardt(engine, scale_factor)
    if on_state is not None:
        on_state(lm.E)
    while True:
        E_, reprojection_error_delta = lm.iterate()
        if on_state is not None:
            on_state(E_)
        if verbose:
            print(f"Iteration {lm.count}: reprojection_error_delta = {reprojection_error_delta}")
        if reprojection_error_delta <= delta_tol or lm.count >= max_iter:
            break
        lm.carry_on(E_)
    return E_


def loss_weights(e_px, f0, loss, loss_scale):
    """w = rho'(s) for residuals ``e_px`` (n, 2) in image units: s = |e / f0|^2, b = (loss_scale / f0)^2 (include/mvba.h)."""
    code, scale = check_loss(loss, loss_scale)
    e = np.asarray(e_px, np.float64).reshape(-1, 2) / f0
    s = (e * e).sum(axis=1)
    if code == 0:
        return np.ones_like(s)
    b = (scale / f0) ** 2
    if code == 1:
        return np.where(s <= b, 1.0, np.sqrt(b / np.maximum(s, b)))
    return 1.0 / (1.0 + s / b)


class BundleAdjuster:
    def __init__(
        self,
        x: npt.NDArray,
        init_X: npt.NDArray | None,
        init_K: npt.NDArray,
        init_R: npt.NDArray,
        init_t: npt.NDArray,
        f0: float = 1.0,
        visibility_index: npt.NDArray | None = None,
        axis: str = "x-right_z-forward",
        loss: str = "squared",
        loss_scale: float | None = None,
        hold=None,
        share=None,
        share_groups=None,
        hold_points=None,
    ):
        """``loss``: "squared" (the reference's sum of squares), "huber" or "cauchy" -- a robust loss with scale
        ``loss_scale`` (delta, in the units of ``x``: pixels), required for the robust ones.
        ``hold`` / ``share`` / ``share_groups``: which camera parameters are adjusted (``parameter_map``):
        ``hold="intrinsics"`` for calibrated cameras, ``share="intrinsics"`` when one camera body took all the images
        (``share_groups`` for a rig of several), ``hold="pose"`` / ``"cameras"`` to refine the structure only.  Tied
        parameters must start equal (``init_K[:, 0, 0]``, ``init_K[:, :2, 2]`` within a group).  A held pose is held in
        the gauge frame BA works in, i.e. relative to camera 0 and the camera-0/1 baseline: the output poses equal the
        input poses up to the rounding of the frame change.
        ``hold_points``: points that are not adjusted -- control points, or the structure that is already
        good when new cameras and points are adjusted against it: a bool array (N,), True = held, or an array of point
        indices; ``hold="points"`` (alone or among the other names) holds all of them: the cameras are refined against
        known structure.  Held points keep their ``init_X`` rows bit for bit, their observations still count in the cost,
        and they are held whole (no per-coordinate mask).  They are held in the gauge frame as held poses are: camera 0 and
        the camera-0/1 baseline component stay fixed however many points are held, so control points that disagree with
        camera 0's initial pose cannot pull it.  Needs ``init_X``, finite at the held rows.
        ``init_X=None``: the points start from their triangulation from the initial cameras, on the device
        (``HipEngine.triangulate``); ValueError if a point cannot be triangulated (seen once, no parallax,
        at infinity) -- ``lib.initialization.triangulate_points`` tells which, to filter the list first."""
        check_loss(loss, loss_scale)  # (ValueError before any work)
        x = np.asarray(x)
        hold = self._check_hold_points(x.shape[0], hold, hold_points, init_X)
        self._check_map(x.shape[1], axis, init_K, hold, share, share_groups)
        pt_ptr, cam_idx, xy = dense_to_observations(x, visibility_index)
        self._setup(x.shape[0], x.shape[1], pt_ptr, cam_idx, xy, init_X, init_K, init_R, init_t, f0, axis, loss=loss,
                    loss_scale=loss_scale)

    @classmethod
    def from_observations(cls, n_points, n_images, pt_ptr, cam_idx, xy, init_X, init_K, init_R, init_t,
                          f0: float = 1.0, axis: str = "x-right_z-forward", loss: str = "squared",
                          loss_scale: float | None = None, hold=None, share=None, share_groups=None, hold_points=None,
                          **engine_kw):
        """Extension for sizes where the dense (N,m,2) array cannot exist
        (SURVEY 8f rank 1): observation list in CSR-by-point form.  ``loss`` / ``loss_scale`` / ``hold`` / ``share`` /
        ``share_groups`` / ``hold_points`` / ``init_X=None``: as for the constructor."""
        check_loss(loss, loss_scale)
        self = cls.__new__(cls)
        hold = self._check_hold_points(n_points, hold, hold_points, init_X)
        self._check_map(n_images, axis, init_K, hold, share, share_groups)
        self._setup(n_points, n_images, pt_ptr, cam_idx, xy, init_X, init_K, init_R, init_t, f0, axis, loss=loss,
                    loss_scale=loss_scale, **engine_kw)
        return self

    # -- construction ------------------------------------------------------
    _map = None  # (col, n_free) when hold / share were given (set by _check_map before any device work)

    _held = None  # bool (N,) when points are held (set by _check_hold_points before any device work)

    def _check_hold_points(self, n_points, hold, hold_points, init_X):
        """The point mask of ``hold_points`` and of the name "points" in ``hold``; returns ``hold`` without that name (None
        if nothing is left), for parameter_map.  ValueErrors before any device work."""
        names = None
        if isinstance(hold, str):
            names = [hold]
        elif hold is not None and not isinstance(hold, np.ndarray) and len(hold) and all(isinstance(v, str) for v in hold):
            names = list(hold)
        all_points = names is not None and "points" in names
        if all_points:
            names = [nm for nm in names if nm != "points"]
            hold = names if names else None
        if hold_points is None and not all_points:
            return hold
        if init_X is None:
            raise ValueError(f"hold_points with init_X=None: the {int(n_points)} points would start from their triangulation, and a "
                             f"held point stays where init_X puts it")
        X = np.asarray(init_X, dtype=np.float64)
        if X.shape != (int(n_points), 3):
            raise ValueError(f"hold_points: init_X must have shape ({int(n_points)}, 3), got {X.shape}")
        mask = np.zeros(int(n_points), dtype=bool) if hold_points is None else point_hold_mask(n_points, hold_points)
        if all_points:
            mask[:] = True
        mask = point_hold_mask(n_points, mask, X)  # (the finite check, on the union)
        if mask.any():
            self._held = mask
            self._held_X = X[mask].copy()
        return hold

    @property
    def n_held_points(self) -> int:
        """Points that are not adjusted (``hold_points``)."""
        return 0 if self._held is None else int(self._held.sum())

    def _check_map(self, n_images, axis, init_K, hold, share, share_groups):
        """parameter_map of the constructor's arguments and the check that tied parameters start equal: ValueErrors
        before any device work."""
        if hold is None and share is None:
            if share_groups is not None:
                raise ValueError("share_groups without share")
            return
        if axis not in AXES:
            raise ValueError()
        col, n_free = parameter_map(n_images, axis, hold, share, share_groups)
        K = np.asarray(init_K, dtype=np.float64)
        start = np.stack([K[:, 0, 0], K[:, 0, 2], K[:, 1, 2]], axis=1)  # (m, 3): f, u, v
        labels = np.zeros(int(n_images), dtype=np.int64) if share_groups is None else np.asarray(share_groups)
        for j in np.unique(col[col >= 0]):
            slots = np.nonzero(col == j)[0]
            if len(slots) > 1:
                v = start[slots // 9, slots % 9]
                if not np.all(v == v[0]):
                    raise ValueError(f"group {int(labels[slots[0] // 9])}: shared {SLOT_LABELS[slots[0] % 9]!r} starts from different values "
                                     f"({v.min()!r} .. {v.max()!r})")
        self._map = (col, n_free)

    @property
    def n_free_camera_parameters(self) -> int:
        """Unknowns of the reduced camera system: 9 m - 7 by default, fewer with hold / share."""
        return 9 * self._n_images - 7 if self._map is None else int(self._map[1])

    def _make_engine(self, n_points, n_images, pt_ptr, cam_idx, xy, f0, axis, **kw):
        from ._mvba import HipEngine

        return HipEngine(n_points, n_images, pt_ptr, cam_idx, xy, f0, axis, **kw)

    def _setup(self, n_points, n_images, pt_ptr, cam_idx, xy, init_X, init_K, init_R, init_t, f0, axis, loss="squared",
               loss_scale=None, **engine_kw):
        self._loss, self._loss_scale = loss, loss_scale
        if loss != "squared":  # (the squared loss keeps the engine's plain constructor call)
            engine_kw = dict(engine_kw, loss=loss, loss_scale=loss_scale)
        triangulate = init_X is None  # (the gauge transform of the cameras needs cameras 0 and 1 alone)
        init_X = np.zeros((0, 3)) if triangulate else np.asarray(init_X, dtype=np.float64)
        init_K = np.asarray(init_K, dtype=np.float64)
        init_R, init_t = np.asarray(init_R, dtype=np.float64), np.asarray(init_t, dtype=np.float64)
        # camera-0 pose and baseline length for the way back (ref :23-33)
        if axis == "x-right_z-forward":
            c0c1_len = np.abs(init_R[0, :, 0] @ (init_t[1] - init_t[0]))
        elif axis == "x-up_z-forward":
            c0c1_len = np.abs(init_R[0, :, 1] @ (init_t[1] - init_t[0]))
        else:
            raise ValueError()
        self._init_camera0_params = {"R": init_R[0], "t": init_t[0], "c0c1_len": c0c1_len}
        X, R, t = to_gauge_frame(init_X, init_R, init_t, axis)
        self._f0 = f0
        self._n_points, self._n_images = int(n_points), int(n_images)
        self._engine = self._make_engine(self._n_points, self._n_images, pt_ptr, cam_idx, xy, f0, axis, **engine_kw)
        if triangulate:
            X = np.zeros((self._n_points, 3))
        self._engine.set_params(X, init_K[:, 0, 0], init_K[:, :2, 2], t, R)  # ref :45-48
        if triangulate:
            _, status, _ = self._engine.triangulate()
            bad = np.nonzero(np.asarray(status) != 0)[0]
            if len(bad):
                self._engine.close()  # (its device buffers go now, not at garbage collection)
                raise ValueError(f"init_X=None: {len(bad)} of {self._n_points} points cannot be triangulated from the initial cameras "
                                 f"(first: point {int(bad[0])}, status {int(status[bad[0]])}: 1 fewer than two observations, 2 no "
                                 f"parallax, 3 at infinity); filter them with lib.initialization.triangulate_points")
        if self._map is not None:
            self._engine.set_parameter_map(self._map[0], self._map[1])
        if self._held is not None:
            self._engine.set_point_hold(self._held)
        self._engine_frame = "gauge"  # the frame of the engine's state: "input" once optimize() has applied the way back
        self._log: list[dict[str, npt.NDArray | float]] = []

    # -- the reference's public methods --------------------------------------
    def optimize(
        self,
        scale_factor: float = 10.0,
        delta_tol: float = 1e-8,
        max_iter: int = 100,
        is_debug: bool = False,
    ) -> tuple[npt.NDArray, npt.NDArray, npt.NDArray, npt.NDArray]:
        on_state = None
        if is_debug:
            self._log.clear()  # ref :90
            self._log_errors = []
            self._engine.snapshot_clear()
            # The log lives in device memory while optimize() runs: 24 N + 120 m bytes per outer iteration (24 MB at
            # 1 M points, 240 MB at 10 M), one device-to-device copy on the engine's stream per entry.  Above
            # MVBA_LOG_DEVICE_BYTES (default 16 GiB), or when the device cannot allocate the next slab, the entries
            # gathered so far are fetched to the host (as get_log() would) and the device log starts over.
            entry_bytes = 24 * self._n_points + 120 * self._n_images
            budget = int(os.environ.get("MVBA_LOG_DEVICE_BYTES", str(16 << 30)))

            def on_state(err):  # log entries are copies, normalised frame (ref :91-97, :175-183)
                if (len(self._log_errors) + 1) * entry_bytes > budget and self._log_errors:
                    self._fetch_log()
                try:
                    self._engine.snapshot()
                except RuntimeError:  # out of device memory for the next slab
                    if not self._log_errors:
                        raise
                    self._fetch_log()
                    self._engine.snapshot()
                self._log_errors.append(err)

        lm_loop(self._engine, scale_factor, delta_tol, max_iter, on_state)
        # the reference rebinds its state to the de-normalised values (:198-200): the engine applies
        # the way back (:242-258) to its committed state on the device, then hands it over
        cam0 = self._init_camera0_params
        self._engine.apply_similarity(cam0["R"], cam0["t"], cam0["c0c1_len"])
        self._engine_frame = "input"
        X, f, u, t, R = self._engine.get_params()
        if self._held is not None:
            # held in the gauge frame, bit for bit; the way there and back costs rounding: the caller gets the rows it gave
            X[self._held] = self._held_X
        return X, intrinsics_from(f, u, self._f0), R, t

    def covariance(self, scale: str = "unit", frame: str = "input", full_cameras: bool = False) -> dict[str, Any]:
        """Marginal covariances of the current estimate (after optimize(): the solution): ``points`` (N, 3, 3),
        ``cameras`` (m, 9, 9) in the order f, u, v, t, omega, and ``cameras_full`` (9m, 9m) when ``full_cameras``.
        Undamped, with the seven gauge parameters fixed (camera 0's t and omega, one component of camera 1's t: zero rows
        and columns).  With ``hold`` / ``share``: zero rows and columns for every held parameter, identical ones for tied
        parameters, and sigma^2 with 3N + n_free unknowns.  With ``hold_points``: zero 3 x 3 blocks at the held points, the
        camera blocks of the problem with those points fixed, and sigma^2 with 3 (N - n_held) + n_free unknowns.  ``scale="unit"``: (J^T J)^-1 with J in units x / f0; ``"residual"``: times sigma^2 =
        E / (2 n_obs - (3N + 9m - 7)) (also returned as ``sigma2``).  ``frame="gauge"``: the normalised frame BA works in;
        ``"input"``: the caller's frame (omega as a rotation increment R <- Rod(omega) R in that frame).  The engine's
        state is left bitwise as it was.  Raises LinAlgError for a degenerate problem (a point seen once, a camera with
        too few points) -- a held point seen once is legal."""
        if scale not in ("unit", "residual") or frame not in ("input", "gauge"):
            raise ValueError("scale must be 'unit' or 'residual', frame 'input' or 'gauge'")
        if self._loss != "squared":
            raise NotImplementedError(f"covariance() is defined for the squared loss only (this adjuster uses loss={self._loss!r})")
        eng, cam0 = self._engine, self._init_camera0_params
        nf = {} if self._map is None else {"n_free": self._map[1]}
        if self._held is not None:
            nf["n_held"] = self.n_held_points
        if scale == "residual":
            residual_variance(0.0, eng.n_obs, self._n_points, self._n_images, **nf)  # (no redundancy: ValueError before any work)
        saved = None
        if self._engine_frame == "input":  # the covariance is taken in the gauge frame the parameterisation fixes
            saved = eng.get_params()
            X, f, u, t, R = saved
            Xg, Rg, tg = from_gauge_frame_inverse(cam0, X, R, t)
            eng.set_params(Xg, f, u, tg, Rg)
        try:
            E = eng.cost() if scale == "residual" else None
            cov = eng.covariance(points=True, cameras=True, full=full_cameras)
        finally:
            if saved is not None:
                eng.set_params(*saved)
        out: dict[str, Any] = {"points": cov["points"], "cameras": cov["cameras"], "timings_ms": cov["timings_ms"]}
        if full_cameras:
            out["cameras_full"] = cov["cameras_full"]
        if frame == "input":
            out["points"], out["cameras"], Cf = covariance_to_input_frame(cam0, out["points"], out["cameras"], out.get("cameras_full"))
            if full_cameras:
                out["cameras_full"] = Cf
        if scale == "residual":
            s2 = residual_variance(E, eng.n_obs, self._n_points, self._n_images, **nf)
            out["sigma2"] = s2
            for k in ("points", "cameras", "cameras_full"):
                if k in out:
                    out[k] = out[k] * s2
        return out

    def residuals(self) -> npt.NDArray:
        """(n_obs, 2) reprojection residuals in image units (projection minus observation) at the current estimate, in
        the engine's observation order -- for the dense constructor the point-major order of dense_to_observations
        (visible observations only).  The same in either frame."""
        return self._engine.residuals()

    def weights(self) -> npt.NDArray:
        """(n_obs,) IRLS weights w_o = rho'(|e_o|^2) of the loss at the current estimate (1 for the squared loss):
        below 1 where the robust loss discounts an observation, e.g. ``weights() > 0.5`` as an inlier mask."""
        return loss_weights(self.residuals(), self._f0, self._loss, self._loss_scale)

    def _fetch_log(self):
        """Device-resident log entries -> host dicts (in order), device log emptied."""
        for i, err in enumerate(self._log_errors):
            X, _, _, t, R = self._engine.snapshot_read(i)
            self._log.append({"points": X, "basis": R, "pos": t, "reprojection_error": err})
        self._log_errors = []
        self._engine.snapshot_clear()

    def get_log(self) -> list[dict[str, npt.NDArray | float]]:
        """ref :204-206.  The per-iteration states were kept in device memory while optimize(is_debug=True) ran
        (`mvba_snapshot`, 24 N + 120 m bytes each); they cross PCIe here, once, the first time the log is asked
        for.  (The device log belongs to this adjuster's engine: code that drives `_engine.snapshot*` itself between
        optimize() and get_log() -- bench.py's episode restarts do, without is_debug -- would replace its entries.)"""
        if getattr(self, "_log_errors", None):
            self._fetch_log()
        return self._log
