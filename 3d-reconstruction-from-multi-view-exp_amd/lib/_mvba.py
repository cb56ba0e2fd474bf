"""ctypes binding of libmvba.so (include/mvba.h) -- the only way into the HIP engine.

There is NO CPU fallback here: if the library is missing, or there is no GPU,
construction raises.  (The NumPy restatement lives in ``oracle/`` and is test
infrastructure only.)
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVBA_LIBRARY", os.path.join(os.path.dirname(_HERE), "libmvba.so"))

MVBA_OK, MVBA_ERR_BADARG, MVBA_ERR_SINGULAR, MVBA_ERR_HIP, MVBA_ERR_RCCL, MVBA_ERR_STATE = range(6)

KERNEL_IDS = ("resid_jac", "point_blocks", "point_inv", "schur", "allreduce", "solve", "backsub_cost", "cost")
BUF = {"residual": 0, "JX": 1, "JC": 2, "E": 3, "dP": 4, "A_full": 5, "b_full": 6, "dxi": 7, "dX": 8,
       "trial_X": 9, "trial_cam": 10, "index_k": 11, "index_l": 12, "index_a": 13, "index_seg": 14, "weight": 15}
LOSSES = {"squared": 0, "huber": 1, "cauchy": 2}  # mvba_create_robust's loss codes (MVBA_LOSS_*)


def check_loss(loss, loss_scale):
    """(loss code, scale) for mvba_create_robust; ValueError on a bad pair (before any library call).
    ``loss_scale`` (delta, image units) is required for a robust loss and ignored for the squared one."""
    if not isinstance(loss, str) or loss not in LOSSES:
        raise ValueError(f"loss must be one of {sorted(LOSSES)}, got {loss!r}")
    if loss == "squared":
        return 0, 0.0
    if loss_scale is None:
        raise ValueError(f"loss={loss!r} needs loss_scale (delta in image units)")
    try:
        scale = float(loss_scale)
    except (TypeError, ValueError):
        raise ValueError(f"loss_scale must be a number, got {loss_scale!r}") from None
    if not np.isfinite(scale) or scale <= 0.0:
        raise ValueError(f"loss_scale must be finite and > 0, got {loss_scale!r}")
    return LOSSES[loss], scale

_dp = C.POINTER(C.c_double)


class Problem(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("n_obs", C.c_int64), ("n_images", C.c_int32),
                ("gauge_axis", C.c_int32), ("pt_ptr", C.POINTER(C.c_int64)),
                ("cam_idx", C.POINTER(C.c_int32)), ("xy", _dp), ("f0", C.c_double),
                ("device", C.c_int32), ("xy_layout", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("ms", C.c_double * 16), ("launches", C.c_int64 * 16),
                ("n_linearize", C.c_int64), ("n_try_step", C.c_int64), ("n_commit", C.c_int64),
                ("n_lu_fallback", C.c_int64), ("n_barrier_fallback", C.c_int64)]


# every symbol include/mvba.h declares: (restype, argtypes)
SIGNATURES = {
    "mvba_version": (C.c_char_p, []),
    "mvba_last_error": (C.c_char_p, []),
    "mvba_kernel_name": (C.c_char_p, [C.c_int32]),
    "mvba_device_count": (C.c_int, [C.POINTER(C.c_int32)]),
    "mvba_create": (C.c_int, [C.POINTER(Problem), C.POINTER(C.c_void_p)]),
    "mvba_create_robust": (C.c_int, [C.POINTER(Problem), C.c_int32, C.c_double, C.POINTER(C.c_void_p)]),
    "mvba_destroy": (None, [C.c_void_p]),
    "mvba_set_params": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _dp]),
    "mvba_get_params": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _dp]),
    "mvba_apply_similarity": (C.c_int, [C.c_void_p, _dp, _dp, C.c_double]),
    "mvba_snapshot": (C.c_int, [C.c_void_p]),
    "mvba_snapshot_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mvba_snapshot_read": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp, _dp]),
    "mvba_snapshot_clear": (C.c_int, [C.c_void_p]),
    "mvba_snapshot_restore": (C.c_int, [C.c_void_p, C.c_int64]),
    "mvba_cost": (C.c_int, [C.c_void_p, _dp]),
    "mvba_linearize": (C.c_int, [C.c_void_p]),
    "mvba_try_step": (C.c_int, [C.c_void_p, C.c_double, _dp]),
    "mvba_commit": (C.c_int, [C.c_void_p]),
    "mvba_set_parameter_map": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]),
    "mvba_set_point_hold": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8)]),
    "mvba_covariance": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp]),
    "mvba_residuals": (C.c_int, [C.c_void_p, _dp]),
    "mvba_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "mvba_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "mvba_reset_stats": (C.c_int, [C.c_void_p]),
    "mvba_get_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mvba_comm_unique_id": (C.c_int, [C.c_void_p]),
    "mvba_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "mvba_comm_init_host": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "mvba_debug_read": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int64, C.POINTER(C.c_int64)]),
    "mvba_host_obs_math": (C.c_int, [_dp, _dp, _dp, C.c_double, _dp]),
    "mvba_triangulate": (C.c_int, [_dp, _dp, _dp, C.c_int32, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int64,
                                   C.c_int32, _dp, _dp, C.POINTER(C.c_int32), _dp, C.c_int32]),
    "mvba_triangulate_state": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.POINTER(C.c_int32), _dp]),
    "mvba_resect": (C.c_int, [_dp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int64, C.c_int32,
                              C.POINTER(C.c_uint8), _dp, _dp, C.POINTER(C.c_int32), _dp, C.c_int32]),
    "mvba_covisibility": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64),
                                    _dp, C.c_int32]),
    "mvba_two_view": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int64, C.POINTER(C.c_int32),
                                C.c_int32, _dp, _dp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int32]),
    "mvba_two_view_robust": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int64, C.POINTER(C.c_int32),
                                       C.c_int32, C.c_double, C.c_int32, C.c_uint64, C.c_int32, _dp, _dp, C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), _dp, C.c_int32]),
    "mvba_ransac_sample": (C.c_int, [C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    "mvba_homography_robust": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int64, C.POINTER(C.c_int32),
                                         C.c_int32, C.c_double, C.c_int32, C.c_uint64, C.c_int32, _dp, _dp, C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), _dp, C.c_int32]),
    "mvba_homography_sample": (C.c_int, [C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    "mvba_resect_robust": (C.c_int, [_dp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int64, C.c_int32,
                                     C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.c_int32, C.c_double, C.c_int32, C.c_uint64, C.c_int32,
                                     _dp, _dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, C.c_int32]),
    "mvba_resect_sample": (C.c_int, [C.c_uint64, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    "mvba_pose_robust": (C.c_int, [_dp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int64, C.c_int32,
                                   C.POINTER(C.c_uint8), _dp, C.POINTER(C.c_int32), C.c_int32, C.c_double, C.c_int32, C.c_uint64,
                                   C.c_int32, C.c_int32, _dp, _dp, _dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, C.c_int32]),
    "mvba_pose_refine": (C.c_int, [_dp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int64, C.c_int32,
                                   C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _dp, C.POINTER(C.c_int32), C.c_int32, C.c_int32, _dp, _dp,
                                   _dp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int32]),
    "mvba_pose_sample": (C.c_int, [C.c_uint64, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    "mvba_triangulate_robust": (C.c_int, [_dp, _dp, _dp, C.c_int32, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int64,
                                          C.c_double, C.c_int32, C.c_uint64, C.c_int32, C.c_int32, _dp, _dp, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), _dp,
                                          C.c_int32]),
    "mvba_triangulate_sample": (C.c_int, [C.c_uint64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "mvba_align_robust": (C.c_int, [C.c_int64, _dp, _dp, C.POINTER(C.c_uint8), C.c_int32, C.c_double, C.c_int32, C.c_uint64, C.c_int32, _dp, _dp,
                                    C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, C.c_int32]),
    "mvba_align": (C.c_int, [C.c_int64, _dp, _dp, C.POINTER(C.c_uint8), C.c_int32, _dp, _dp, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                             C.c_int32]),
    "mvba_align_sample": (C.c_int, [C.c_uint64, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    "mvba_build_tracks": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), _dp, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_uint8), C.c_int32,
                                    C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int64), _dp, C.c_int32]),
    "mvba_match_descriptors": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                         C.c_double, C.c_int32, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), _dp,
                                         C.c_int32]),
    "mvba_project": (C.c_int, [_dp, C.c_int64, _dp, _dp, _dp, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                               C.c_int64, _dp, C.c_int32]),
    "mvsvd_factorize": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_int32]),
    "mvsvd_create": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "mvsvd_load": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mvsvd_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _dp]),
    "mvsvd_load_images": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32]),
    "mvsvd_load_base": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mvsvd_load_base_images": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_double]),
    "mvsvd_run_scaled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, _dp]),
    "mvsvd_depth_begin": (C.c_int, [C.c_void_p, C.c_int32]),
    "mvsvd_depth_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, _dp, _dp]),
    "mvsvd_depth_read": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mvsvd_destroy": (None, [C.c_void_p]),
}

_lib = None


def load_library():
    """dlopen libmvba.so (loudly) and attach the prototypes."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libmvba.so not found at {LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (or make -C 3d-reconstruction-from-multi-view-exp_amd/csrc). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _as(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def raise_for(rc, lib=None):
    if rc == MVBA_OK:
        return
    msg = (lib or load_library()).mvba_last_error().decode()
    if rc == MVBA_ERR_SINGULAR:
        raise np.linalg.LinAlgError(msg)  # ref :128 / :146 raise numpy.linalg.LinAlgError
    if rc == MVBA_ERR_BADARG:
        raise ValueError(msg)  # ref :27-28
    raise RuntimeError(f"libmvba error {rc}: {msg}")


def device_count():
    lib = load_library()
    n = C.c_int32(0)
    rc = lib.mvba_device_count(C.byref(n))
    return n.value if rc == MVBA_OK else 0


def _require_device(name):
    if device_count() < 1:
        raise RuntimeError(f"libmvba: no HIP device visible; {name} has no CPU fallback")


def _obs_list(pt_ptr, cam_idx, xy, m, n_points=None):
    """An observation list as the C entry points take it: ``(n, n_obs, pt_ptr pointer, cam_idx pointer, xy)``.  With
    ``pt_ptr=None`` the dense grid (null pointers; xy (N, m, 2), or ``n_points`` where there is no xy); otherwise xy comes
    back as (n_obs, 2).  ``n_points``, where the caller knows it, must agree."""
    if pt_ptr is None:
        if xy is None:
            assert n_points is not None
            n = int(n_points)
        else:
            assert xy.ndim == 3 and xy.shape[1:] == (m, 2) and n_points in (None, xy.shape[0])
            n = xy.shape[0]
        return n, n * m, None, None, xy
    pt_ptr, cam_idx = _as(pt_ptr, np.int64), _as(cam_idx, np.int32)
    n, n_obs = pt_ptr.shape[0] - 1, cam_idx.shape[0]
    assert n_points is None or int(n_points) == n
    if xy is not None:
        xy = xy.reshape(-1, 2)
        assert xy.shape[0] == n_obs
    # (a ctypes pointer made by data_as keeps its array alive)
    return n, n_obs, pt_ptr.ctypes.data_as(C.POINTER(C.c_int64)), cam_idx.ctypes.data_as(C.POINTER(C.c_int32)), xy


def _point_ok_ptr(point_ok, n):
    """``point_ok`` (n,) as bytes and the pointer a call takes: ``(array, pointer)``, both None for ``point_ok=None``.  The
    array comes back with the pointer because it has to stay alive until the call has returned."""
    if point_ok is None:
        return None, None
    ok = _as(np.asarray(point_ok) != 0, np.uint8)
    assert ok.shape == (n,)
    return ok, ok.ctypes.data_as(C.POINTER(C.c_uint8))


def _seed64(seed):
    """A seed as the C interface takes it: modulo 2^64."""
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _timings3(tm):
    return dict(zip(("upload", "kernel", "download"), tm.tolist()))


class HipEngine:
    """Device-resident BA state + kernels.  Protocol (shared with the oracle's
    engine): set_params / get_params / cost / linearize / try_step / commit.
    ``loss`` ("squared", "huber", "cauchy") and ``loss_scale`` (delta in image units) choose the robust loss, fixed
    for the engine's life (include/mvba.h, mvba_create_robust)."""

    def __init__(self, n_points, n_images, pt_ptr, cam_idx, xy, f0, axis, device=-1, loss="squared", loss_scale=None):
        from .bundle_adjustment import AXES  # local import: avoid a cycle

        if axis not in AXES:
            raise ValueError()
        loss_code, scale = check_loss(loss, loss_scale)
        self.loss, self.loss_scale = loss, (scale if loss_code else None)
        self.lib = load_library()
        if device_count() < 1:
            raise RuntimeError("libmvba: no HIP device visible; the BA engine has no CPU fallback")
        self.n, self.m = int(n_points), int(n_images)
        self._pt_ptr = _as(pt_ptr, np.int64)
        self._cam = _as(cam_idx, np.int32)
        self._xy = _as(xy, np.float64)
        planes = self._xy.ndim == 3  # (m, N, 2) image planes of a fully visible scene (xy_layout 1) instead of (n_obs, 2)
        if planes and self._xy.shape != (self.m, self.n, 2):
            raise ValueError("xy as image planes must be (n_images, n_points, 2)")
        if not planes:
            self._xy = self._xy.reshape(-1, 2)
        self.n_obs = int(self._cam.shape[0])
        prob = Problem(self.n, self.n_obs, self.m, AXES[axis],
                       self._pt_ptr.ctypes.data_as(C.POINTER(C.c_int64)),
                       self._cam.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(self._xy), float(f0), int(device), int(planes))
        h = C.c_void_p()
        if loss_code or loss_scale is not None:  # (squared with a scale: through mvba_create_robust, which is mvba_create then)
            raise_for(self.lib.mvba_create_robust(C.byref(prob), loss_code, scale, C.byref(h)), self.lib)
        else:
            raise_for(self.lib.mvba_create(C.byref(prob), C.byref(h)), self.lib)
        self._h = h
        self.n_solves = 0
        self.n_free = 9 * self.m - 7  # unknowns of the reduced camera system (set_parameter_map)
        self.n_held_points = 0  # points that are not unknowns (set_point_hold)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mvba_destroy(self._h)
            self._h = None

    __del__ = close

    def set_params(self, X, f, u, t, R):
        X, f, u, t, R = (_as(v, np.float64) for v in (X, f, u, t, R))
        assert X.shape == (self.n, 3) and f.shape == (self.m,) and u.shape == (self.m, 2)
        assert t.shape == (self.m, 3) and R.shape == (self.m, 3, 3)
        raise_for(self.lib.mvba_set_params(self._h, _ptr(X), _ptr(f), _ptr(u), _ptr(t), _ptr(R)), self.lib)

    def get_params(self):
        X = np.empty((self.n, 3)); f = np.empty(self.m); u = np.empty((self.m, 2))
        t = np.empty((self.m, 3)); R = np.empty((self.m, 3, 3))
        raise_for(self.lib.mvba_get_params(self._h, _ptr(X), _ptr(f), _ptr(u), _ptr(t), _ptr(R)), self.lib)
        return X, f, u, t, R

    # -- debug log (ref :89-98, :175-183): copies of the committed state kept on the device
    def snapshot(self):
        raise_for(self.lib.mvba_snapshot(self._h), self.lib)

    def snapshot_count(self):
        n = C.c_int64()
        raise_for(self.lib.mvba_snapshot_count(self._h, C.byref(n)), self.lib)
        return n.value

    def snapshot_read(self, i):
        X = np.empty((self.n, 3)); f = np.empty(self.m); u = np.empty((self.m, 2))
        t = np.empty((self.m, 3)); R = np.empty((self.m, 3, 3))
        raise_for(self.lib.mvba_snapshot_read(self._h, int(i), _ptr(X), _ptr(f), _ptr(u), _ptr(t), _ptr(R)), self.lib)
        return X, f, u, t, R

    def snapshot_clear(self):
        raise_for(self.lib.mvba_snapshot_clear(self._h), self.lib)

    def snapshot_restore(self, i):
        """Log entry i becomes the committed state again (set_params from device memory)."""
        raise_for(self.lib.mvba_snapshot_restore(self._h, int(i)), self.lib)

    def apply_similarity(self, R0, t0, scale):
        """Committed state -> scale * X R0^T + t0 (likewise t), R0 R, on the device (ref :242-258)."""
        R0, t0 = _as(R0, np.float64), _as(t0, np.float64)
        assert R0.shape == (3, 3) and t0.shape == (3,)
        raise_for(self.lib.mvba_apply_similarity(self._h, _ptr(R0), _ptr(t0), float(scale)), self.lib)

    def cost(self):
        E = C.c_double()
        raise_for(self.lib.mvba_cost(self._h, C.byref(E)), self.lib)
        return E.value

    def linearize(self):
        raise_for(self.lib.mvba_linearize(self._h), self.lib)

    def try_step(self, c):
        E = C.c_double()
        raise_for(self.lib.mvba_try_step(self._h, float(c), C.byref(E)), self.lib)
        self.n_solves += 1
        return E.value

    def commit(self):
        raise_for(self.lib.mvba_commit(self._h), self.lib)

    def set_parameter_map(self, col, n_free=None):
        """Which camera parameters a trial adjusts (include/mvba.h, mvba_set_parameter_map): ``col`` (9m,) int, slot
        9k + p (p: f, u, v, t, omega) -> reduced unknown, -1 = held, equal entries = tied; ``None`` = the default map
        (the seven gauge slots held).  ``n_free`` defaults to ``col.max() + 1``.  Voids the trial, keeps the
        linearisation.  Sharded engines: every rank sets the same map."""
        if col is None:
            raise_for(self.lib.mvba_set_parameter_map(self._h, None, 0), self.lib)
            self.n_free = 9 * self.m - 7
            return
        col = _as(col, np.int32).reshape(-1)
        if col.shape != (9 * self.m,):
            raise ValueError(f"col must have 9 n_images = {9 * self.m} entries, got {col.shape[0]}")
        if n_free is None:
            n_free = int(col.max()) + 1 if col.size else 0
        raise_for(self.lib.mvba_set_parameter_map(self._h, col.ctypes.data_as(C.POINTER(C.c_int32)), int(n_free)), self.lib)
        self.n_free = int(n_free)

    def set_point_hold(self, mask):
        """Which points a trial adjusts (include/mvba.h, mvba_set_point_hold): ``mask`` (n_points,) bool, True = held (not
        an unknown: its step is exactly 0, its residuals still count); ``None`` clears the mask.  Voids the trial, keeps
        the linearisation.  ``triangulate()`` raises while a mask is set.  Sharded engines: the mask of this rank's points."""
        if mask is None:
            raise_for(self.lib.mvba_set_point_hold(self._h, None), self.lib)
            self.n_held_points = 0
            return
        mask = np.asarray(mask)
        if mask.dtype != np.bool_ or mask.shape != (self.n,):
            raise ValueError(f"mask must be a bool array of shape ({self.n},), got {mask.dtype} {mask.shape}")
        m8 = _as(mask, np.uint8)
        raise_for(self.lib.mvba_set_point_hold(self._h, m8.ctypes.data_as(C.POINTER(C.c_uint8))), self.lib)
        self.n_held_points = int(mask.sum())

    def covariance(self, points=True, cameras=True, full=False):
        """Unit marginal covariances (J^T J)^-1 at the committed state, in the engine's frame, gauge parameters fixed
        (zero rows / columns): ``points`` (N, 3, 3), ``cameras`` (m, 9, 9) (f, u, v, t, omega), ``cameras_full``
        (9m, 9m) when ``full``, and ``timings_ms`` (linearise+Schur, factor, inverse, point pass).  Leaves the engine
        linearised at the committed state.  Raises LinAlgError when J^T J is singular (a point seen once, a camera with
        too few points).  With held points (set_point_hold): zero blocks there, and they are never a reason for LinAlgError."""
        P = np.empty((self.n, 6)) if points else None
        Cc = np.empty((self.m, 9, 9)) if cameras else None
        Cf = np.empty((9 * self.m, 9 * self.m)) if full else None
        tm = np.zeros(4)
        raise_for(self.lib.mvba_covariance(self._h, _ptr(P) if P is not None else None, _ptr(Cc) if Cc is not None else None,
                                           _ptr(Cf) if Cf is not None else None, _ptr(tm)), self.lib)
        out = {"timings_ms": dict(zip(("schur", "factor", "inverse", "points"), tm.tolist()))}
        if P is not None:
            i = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
            out["points"] = P[:, i]
        if Cc is not None:
            out["cameras"] = Cc
        if Cf is not None:
            out["cameras_full"] = Cf
        return out

    def triangulate(self, n_refine=2):
        """Replace the committed points by their triangulation from the committed cameras and the engine's own
        observations (mvba_triangulate_state: nothing is uploaded).  Returns ``(quality (n, 3), status (n,), timings_ms)``
        as ``triangulate`` below (the RMS residual in the units of the engine's xy, whatever f0 is); a point whose status is
        not 0 keeps its coordinates.  Voids the linearisation and the
        trial.  Sharded engines: each rank triangulates its own points."""
        q = np.empty((self.n, 3))
        st = np.empty(self.n, np.int32)
        tm = np.zeros(3)
        raise_for(self.lib.mvba_triangulate_state(self._h, int(n_refine), _ptr(q), st.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(tm)),
                  self.lib)
        return q, st, _timings3(tm)

    def residuals(self):
        """(n_obs, 2) residuals f0 e_o in image units at the committed state, in the engine's observation order."""
        e = np.empty((self.n_obs, 2))
        raise_for(self.lib.mvba_residuals(self._h, _ptr(e)), self.lib)
        return e

    # -- measurement / multi-GPU / test hooks
    def set_profiling(self, on):
        """False / True, or 2: time the Schur and residual-Jacobian kernels only."""
        raise_for(self.lib.mvba_set_profiling(self._h, 2 if on == 2 and on is not True else int(bool(on))), self.lib)

    def reset_stats(self):
        raise_for(self.lib.mvba_reset_stats(self._h), self.lib)

    def stats(self):
        s = Stats()
        raise_for(self.lib.mvba_get_stats(self._h, C.byref(s)), self.lib)
        out = {k: {"ms": s.ms[i], "launches": s.launches[i]} for i, k in enumerate(KERNEL_IDS)}
        out["counts"] = {"linearize": s.n_linearize, "try_step": s.n_try_step, "commit": s.n_commit,
                         "lu_fallback": s.n_lu_fallback, "barrier_fallback": s.n_barrier_fallback}
        return out

    def _info(self):
        out = (C.c_int64 * 8)()
        raise_for(self.lib.mvba_get_info(self._h, out), self.lib)
        return list(out)

    def schur_info(self):
        i = self._info()
        # slot form: step-major rows incl. the padding rows of the bounded-skew merge, and the step width = lists per wave
        # (21: k_schur_slots, three lanes per item; 64: k_schur_lanes, one lane per item -- "slots" either way; 0: no slot form)
        return {"items": i[0], "offdiag_items": i[1], "units": i[2], "kernel": ("strip", "pairs", "slots", "dense")[i[3] & 0xff],
                "slot_rows": i[7], "step_width": (i[3] >> 8) & 0xff,
                # slot form: the point ranges of the plan; lane form (step_width 64): the waves of its kernel a CU holds, as the
                # occupancy query answered when the ranges were counted (0 in the other forms)
                "ranges": (i[3] >> 20) & 0xff, "places_per_cu": (i[3] >> 28) & 0xf,
                # the linearisation record: "compact" (64 B: J_X and d/df; lane form, squared loss) or "full" (128 B)
                "record": "compact" if (i[3] >> 16) & 1 else "full",
                # dense form: the workgroups of k_schur_dense = min(chunks, CUs x workgroups per CU); 0 in the other forms
                "workgroups": i[3] >> 32}

    def rccl_version(self):
        i = self._info()
        return {"loaded": i[4], "compiled_against": i[5], "ranks": i[6]}

    def comm_init(self, id128: bytes, rank: int, n_ranks: int):
        buf = C.create_string_buffer(bytes(id128), 128)
        raise_for(self.lib.mvba_comm_init(self._h, buf, int(rank), int(n_ranks)), self.lib)

    def comm_init_host(self, rank: int, n_ranks: int, allreduce):
        """Host-staged transport: ``allreduce(a)`` sums a float64 ndarray in place over the ranks."""
        HOSTFN = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, C.c_int64)

        def _cb(_user, buf, n):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(n,)))
                return 0
            except Exception:  # noqa: BLE001
                return 1

        self._host_cb = HOSTFN(_cb)  # keep the trampoline alive as long as the engine
        raise_for(self.lib.mvba_comm_init_host(self._h, int(rank), int(n_ranks), C.cast(self._host_cb, C.c_void_p), None),
                  self.lib)

    def debug_read(self, name):
        n = C.c_int64()
        raise_for(self.lib.mvba_debug_read(self._h, BUF[name], None, 0, C.byref(n)), self.lib)
        out = np.empty(n.value)
        raise_for(self.lib.mvba_debug_read(self._h, BUF[name], _ptr(out), n.value, C.byref(n)), self.lib)
        return out


def comm_unique_id() -> bytes:
    lib = load_library()
    buf = C.create_string_buffer(128)
    raise_for(lib.mvba_comm_unique_id(buf), lib)
    return buf.raw


def project(X, K, R, t, pt_ptr=None, cam_idx=None, device=-1):
    """Device pinhole projection (mvba_project).  With an observation list (pt_ptr, cam_idx):
    (n_obs, 2); without: the dense grid (N, m, 2).  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_project")
    X, K, R, t = (_as(v, np.float64) for v in (X, K, R, t))
    n, m = X.shape[0], K.shape[0]
    assert X.shape == (n, 3) and K.shape == (m, 3, 3) and R.shape == (m, 3, 3) and t.shape == (m, 3)
    _, n_obs, pp, cp, _ = _obs_list(pt_ptr, cam_idx, None, m, n if pt_ptr is None else None)
    out = np.empty((n, m, 2) if pt_ptr is None else (n_obs, 2))
    raise_for(lib.mvba_project(_ptr(X), n, _ptr(K), _ptr(R), _ptr(t), m, pp, cp, n_obs, _ptr(out), int(device)), lib)
    return out


def triangulate(K, R, t, pt_ptr, cam_idx, xy, n_refine=2, device=-1):
    """Device triangulation of every point from known cameras (mvba_triangulate), the inverse of ``project``.  With an
    observation list (pt_ptr, cam_idx, xy (n_obs, 2)), or ``pt_ptr=None`` and xy (N, m, 2): the dense grid.  xy is in the
    units K projects to: with raw image coordinates and the engine's f, u that is K[2, 2] = 1 (``intrinsics_from`` writes f0
    there, which projects to x / f0).  Returns
    ``X (N, 3), quality (N, 3), status (N,), timings_ms``: status 0 ok, 1 fewer than two observations, 2 no parallax,
    3 at infinity / not finite (X is NaN then); quality = RMS reprojection residual, smallest depth, largest angle between
    two viewing rays (radians).  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_triangulate")
    K, R, t, xy = (_as(v, np.float64) for v in (K, R, t, xy))
    m = K.shape[0]
    assert K.shape == (m, 3, 3) and R.shape == (m, 3, 3) and t.shape == (m, 3)
    n, n_obs, pp, cp, xy = _obs_list(pt_ptr, cam_idx, xy, m)
    X, q, st, tm = np.empty((n, 3)), np.empty((n, 3)), np.empty(n, np.int32), np.zeros(3)
    raise_for(lib.mvba_triangulate(_ptr(K), _ptr(R), _ptr(t), m, n, pp, cp, _ptr(xy), n_obs, int(n_refine), _ptr(X), _ptr(q),
                                   st.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(tm), int(device)), lib)
    return X, q, st, _timings3(tm)


def resect(X, pt_ptr, cam_idx, xy, n_images, point_ok=None, device=-1):
    """Device resection of every camera from known points (mvba_resect): the normalised DLT.  The list as for ``triangulate``
    (``pt_ptr=None`` with xy (N, m, 2): the dense grid).  ``point_ok`` (N,) marks the points to use (default: those whose X
    is finite).  Returns ``P (m, 3, 4)`` -- it projects to the units of the xy given -- with |P[2, :3]| = 1 and
    det P[:, :3] > 0, ``quality (m, 2)`` (RMS reprojection residual, eigenvalue ratio), ``status (m,)`` (0 ok, 1 fewer than 6
    usable observations, 2 degenerate; P is NaN then), ``timings_ms``.  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_resect")
    X, xy = _as(X, np.float64), _as(xy, np.float64)
    n, m = X.shape[0], int(n_images)
    assert X.shape == (n, 3)
    _, n_obs, pp, cp, xy = _obs_list(pt_ptr, cam_idx, xy, m, n)
    ok, okp = _point_ok_ptr(point_ok, n)
    P, q, st, tm = np.empty((m, 3, 4)), np.empty((m, 2)), np.empty(m, np.int32), np.zeros(3)
    raise_for(lib.mvba_resect(_ptr(X), n, pp, cp, _ptr(xy), n_obs, m, okp, _ptr(P), _ptr(q), st.ctypes.data_as(C.POINTER(C.c_int32)),
                              _ptr(tm), int(device)), lib)
    return P, q, st, _timings3(tm)


def covisibility(pt_ptr, cam_idx, n_images, n_points=None, device=-1):
    """Co-visibility counts on the device (mvba_covisibility): ``count (m, m) int64``, count[k, l] = the number of points seen
    in both k and l, count[k, k] = camera k's observation count.  ``pt_ptr=None`` with ``n_points``: the dense grid.  Returns
    ``count, timings_ms``.  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_covisibility")
    m = int(n_images)
    n, n_obs, pp, cp, _ = _obs_list(pt_ptr, cam_idx, None, m, n_points)
    count, tm = np.zeros((max(m, 0), max(m, 0)), np.int64), np.zeros(3)
    raise_for(lib.mvba_covisibility(n, m, pp, cp, n_obs, count.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(tm), int(device)), lib)
    return count, _timings3(tm)


def two_view(pt_ptr, cam_idx, xy, n_images, pairs, device=-1):
    """Fundamental matrices of camera pairs from the points they share (mvba_two_view): the normalised 8-point method.  The
    list as for ``triangulate`` (``pt_ptr=None`` with xy (N, m, 2): the dense grid), ``pairs`` (P, 2) = (k, l).  Returns
    ``F (P, 3, 3)`` -- x_l^T F x_k = 0 in the units of xy, rank 2, |F| = 1, largest entry positive --, ``quality (P, 2)`` (RMS
    Sampson distance, eigenvalue ratio), ``n_shared (P,)``, ``status (P,)`` (0 ok, 1 fewer than 8 shared points, 2 degenerate;
    F and quality are NaN then), ``timings_ms``.  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_two_view")
    xy, m = _as(xy, np.float64), int(n_images)
    pairs = _as(pairs, np.int32).reshape(-1, 2)
    n, n_obs, pp, cp, xy = _obs_list(pt_ptr, cam_idx, xy, m)
    P = pairs.shape[0]
    F, q, ns, st, tm = np.empty((P, 3, 3)), np.empty((P, 2)), np.empty(P, np.int64), np.empty(P, np.int32), np.zeros(3)
    raise_for(lib.mvba_two_view(n, m, pp, cp, _ptr(xy), n_obs, pairs.ctypes.data_as(C.POINTER(C.c_int32)), P, _ptr(F), _ptr(q),
                                ns.ctypes.data_as(C.POINTER(C.c_int64)), st.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(tm), int(device)), lib)
    return F, q, ns, st, _timings3(tm)


def _robust_outputs(model, n_items, count_key, n_hypotheses, inlier_shape, return_counts):
    """What the three ``*_robust`` calls share: the output arrays from ``quality`` on and the dict they come back in.  Returns
    ``(tail, result)``: the C arguments quality, ``count_key`` (n_shared / n_usable), n_inliers, best, inlier, hyp_count, status,
    timings_ms, and a function that builds the result from ``model`` (the call's own arrays) once the call has returned."""
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    q, tm = np.empty((max(n_items, 0), 2)), np.zeros(4)
    cnt, ni, best, st = np.empty(n_items, np.int64), np.empty(n_items, np.int64), np.empty(n_items, np.int32), np.empty(n_items, np.int32)
    inl = None if inlier_shape is None else np.empty(inlier_shape, np.uint8)
    hc = np.empty((n_items, max(n_hypotheses, 0)), np.int32) if return_counts else None
    tail = (_ptr(q), cnt.ctypes.data_as(i64), ni.ctypes.data_as(i64), best.ctypes.data_as(i32),
            None if inl is None else inl.ctypes.data_as(C.POINTER(C.c_uint8)), None if hc is None else hc.ctypes.data_as(i32),
            st.ctypes.data_as(i32), _ptr(tm))

    def result():
        out = {**model, "quality": q, count_key: cnt, "n_inliers": ni, "best": best, "status": st,
               "timings_ms": dict(zip(("upload", "score", "refit", "other"), tm.tolist()))}
        if inl is not None:
            out["inlier"] = inl.astype(bool)
        if hc is not None:
            out["hyp_count"] = hc
        return out

    return tail, result


def _sample(name, n_idx, seed, *index):
    """The ``n_idx`` indices a ``*_sample`` entry point writes for ``seed`` (taken modulo 2^64) and its integer arguments."""
    lib = load_library()
    idx = np.empty(n_idx, np.int64)
    raise_for(getattr(lib, name)(_seed64(seed), *(int(v) for v in index), idx.ctypes.data_as(C.POINTER(C.c_int64))), lib)
    return idx


def _pairs_robust(entry, key, pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses, seed, n_refit, return_inliers, return_counts,
                  device):
    """``two_view_robust`` and ``homography_robust``: the C entry point ``entry``, whose matrices come back under ``key``."""
    lib = load_library()
    _require_device(entry)
    xy, m = _as(xy, np.float64), int(n_images)
    pairs = _as(pairs, np.int32).reshape(-1, 2)
    n, n_obs, pp, cp, xy = _obs_list(pt_ptr, cam_idx, xy, m)
    P, H = pairs.shape[0], int(n_hypotheses)
    M = np.empty((P, 3, 3))
    tail, result = _robust_outputs({key: M}, P, "n_shared", H, (P, n) if return_inliers else None, return_counts)
    raise_for(getattr(lib, entry)(n, m, pp, cp, _ptr(xy), n_obs, pairs.ctypes.data_as(C.POINTER(C.c_int32)), P, float(threshold), H,
                                  _seed64(seed), int(n_refit), _ptr(M), *tail, int(device)), lib)
    return result()


def two_view_robust(pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses=512, seed=0, n_refit=2, return_inliers=True,
                    return_counts=False, device=-1):
    """Fundamental matrices by 8-point RANSAC on the device (mvba_two_view_robust).  The list and ``pairs`` as for ``two_view``;
    ``threshold`` is a Sampson distance in the units of xy.  Returns a dict: ``F (P, 3, 3)``, ``quality (P, 2)`` (RMS Sampson
    distance over the final inliers, eigenvalue ratio of the last kept refit), ``n_shared``, ``n_inliers``, ``best``, ``status``
    (P,) (0 ok, 1 fewer than 8 shared points, 2 every hypothesis degenerate, 4 best count below 8; F and quality NaN then),
    ``inlier (P, N) bool`` (``return_inliers``: P x N bytes on the host and on the device), ``hyp_count (P, H) int32``
    (``return_counts``), ``timings_ms``.  No CPU fallback."""
    return _pairs_robust("mvba_two_view_robust", "F", pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses, seed, n_refit,
                         return_inliers, return_counts, device)


def ransac_sample(seed, k, l, h, n):
    """The 8 distinct indices below ``n`` that hypothesis ``h`` of pair (k, l) draws (mvba_ransac_sample: the host instance of
    the function the kernel runs; no GPU needed)."""
    return _sample("mvba_ransac_sample", 8, seed, k, l, h, n)


def homography_robust(pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses=512, seed=0, n_refit=2, return_inliers=True,
                      return_counts=False, device=-1):
    """Homographies by 4-point RANSAC on the device (mvba_homography_robust).  The arguments of ``two_view_robust``;
    ``threshold`` is a transfer distance in the units of xy, held in both directions.  Returns its dict with ``H (P, 3, 3)`` --
    x_l ~ H x_k, |H| = 1, largest entry positive -- in the place of F; ``quality (P, 2)`` is the RMS symmetric transfer distance
    over the final inliers and the eigenvalue ratio of the last kept refit; ``status`` 0 ok, 1 fewer than 4 shared points, 2
    every hypothesis degenerate, 4 best count below 4.  No CPU fallback."""
    return _pairs_robust("mvba_homography_robust", "H", pt_ptr, cam_idx, xy, n_images, pairs, threshold, n_hypotheses, seed, n_refit,
                         return_inliers, return_counts, device)


def homography_sample(seed, k, l, h, n):
    """The 4 distinct indices below ``n`` that hypothesis ``h`` of pair (k, l) draws (mvba_homography_sample: the host instance
    of the function the kernel runs; no GPU needed)."""
    return _sample("mvba_homography_sample", 4, seed, k, l, h, n)


def resect_robust(X, pt_ptr, cam_idx, xy, n_images, threshold, point_ok=None, cameras=None, n_hypotheses=512, seed=0, n_refit=2,
                  return_inliers=True, return_counts=False, device=-1):
    """Camera matrices by 6-point RANSAC on the device (mvba_resect_robust).  X, the list and ``point_ok`` as for ``resect``;
    ``cameras`` lists the cameras to solve (default: all; duplicates allowed) and every per-camera output is indexed by the
    position in it; ``threshold`` is a reprojection distance in the units of xy.  Returns a dict: ``P (C, 3, 4)``,
    ``quality (C, 2)`` (RMS reprojection residual over the final inliers, eigenvalue ratio of the last kept refit),
    ``n_usable``, ``n_inliers``, ``best``, ``status`` (C,) (0 ok, 1 fewer than 6 usable observations, 2 every hypothesis
    degenerate, 4 best count below 6; P and quality NaN then), ``inlier (n_obs,) bool`` in the order of the list given
    (``return_inliers``), ``hyp_count (C, H) int32`` (``return_counts``), ``timings_ms``.  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_resect_robust")
    X, xy = _as(X, np.float64), _as(xy, np.float64)
    n, m = X.shape[0], int(n_images)
    assert X.shape == (n, 3)
    _, n_obs, pp, cp, xy = _obs_list(pt_ptr, cam_idx, xy, m, n)
    ok, okp = _point_ok_ptr(point_ok, n)
    cams = None if cameras is None else _as(cameras, np.int32).reshape(-1)
    nc, H = m if cams is None else cams.shape[0], int(n_hypotheses)
    P = np.empty((max(nc, 0), 3, 4))
    tail, result = _robust_outputs({"P": P}, nc, "n_usable", H, n_obs if return_inliers else None, return_counts)
    raise_for(lib.mvba_resect_robust(_ptr(X), n, pp, cp, _ptr(xy), n_obs, m, okp, None if cams is None else cams.ctypes.data_as(C.POINTER(C.c_int32)),
                                     nc, float(threshold), H, _seed64(seed), int(n_refit), _ptr(P), *tail, int(device)), lib)
    return result()


def resect_sample(seed, k, h, n):
    """The 6 distinct indices below ``n`` that hypothesis ``h`` of camera ``k`` draws (mvba_resect_sample: the host instance of
    the function the kernel runs; no GPU needed)."""
    return _sample("mvba_resect_sample", 6, seed, k, h, n)


def _pose_args(X, pt_ptr, cam_idx, xy, K, point_ok, cameras):
    """The arguments mvba_pose_robust and mvba_pose_refine share, as ctypes: (keep-alive tuple, n, n_obs, m, pp, cp, xy, okp, K,
    camera pointer, n_cameras)."""
    X, xy, K = _as(X, np.float64), _as(xy, np.float64), _as(K, np.float64)
    n, m = X.shape[0], K.shape[0]
    assert X.shape == (n, 3) and K.shape == (m, 3, 3)
    _, n_obs, pp, cp, xy = _obs_list(pt_ptr, cam_idx, xy, m, n)
    ok, okp = _point_ok_ptr(point_ok, n)
    cams = None if cameras is None else _as(cameras, np.int32).reshape(-1)
    nc = m if cams is None else cams.shape[0]
    return (X, ok, cams), n, n_obs, m, pp, cp, xy, okp, K, None if cams is None else cams.ctypes.data_as(C.POINTER(C.c_int32)), nc


def pose_robust(X, pt_ptr, cam_idx, xy, K, threshold, point_ok=None, cameras=None, n_hypotheses=512, seed=0, n_refine=5, n_refit=2,
                return_inliers=True, return_counts=False, device=-1):
    """Camera poses with known intrinsics by P3P RANSAC and a pose-only refit on the device (mvba_pose_robust).  X, the list,
    ``point_ok`` and ``cameras`` as for ``resect_robust``; ``K (m, 3, 3)`` projects to the units of xy; ``threshold`` is a
    reprojection distance in those units.  Returns a dict: ``R (C, 3, 3)`` (columns = the camera axes), ``t (C, 3)``,
    ``quality (C, 2)`` (RMS reprojection residual over the final inliers, smallest relative Cholesky pivot of the last kept
    refit), ``n_usable``, ``n_inliers``, ``best``, ``status`` (C,) (0 ok, 1 fewer than 4 usable observations, 2 every hypothesis
    degenerate, 4 best count below 4; R, t and quality NaN then), ``inlier (n_obs,) bool`` (``return_inliers``), ``hyp_count
    (C, H) int32`` (``return_counts``), ``timings_ms``.  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_pose_robust")
    keep, n, n_obs, m, pp, cp, xy, okp, K, camp, nc = _pose_args(X, pt_ptr, cam_idx, xy, K, point_ok, cameras)
    H = int(n_hypotheses)
    R, t = np.empty((nc, 3, 3)), np.empty((nc, 3))
    tail, result = _robust_outputs({"R": R, "t": t}, nc, "n_usable", H, n_obs if return_inliers else None, return_counts)
    raise_for(lib.mvba_pose_robust(_ptr(keep[0]), n, pp, cp, _ptr(xy), n_obs, m, okp, _ptr(K), camp, nc, float(threshold), H,
                                   _seed64(seed), int(n_refine), int(n_refit), _ptr(R), _ptr(t), *tail, int(device)), lib)
    return result()


def pose_refine(X, pt_ptr, cam_idx, xy, K, R, t, point_ok=None, obs_ok=None, cameras=None, n_steps=10, device=-1):
    """Gauss-Newton on the poses ``R (C, 3, 3)``, ``t (C, 3)`` of the listed cameras against the fixed points X
    (mvba_pose_refine: the refit of ``pose_robust`` alone); ``obs_ok (n_obs,)`` marks the observations to use.  Returns a dict:
    ``R``, ``t`` (copies; the input pose where status is not 0), ``quality (C, 3)`` (RMS before, after, steps taken),
    ``n_usable``, ``status`` (C,) (0 ok, 1 fewer than 3 observations, 2 singular at the first step or input not finite),
    ``timings_ms``.  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_pose_refine")
    keep, n, n_obs, m, pp, cp, xy, okp, K, camp, nc = _pose_args(X, pt_ptr, cam_idx, xy, K, point_ok, cameras)
    obp = None
    if obs_ok is not None:
        ob = _as(np.asarray(obs_ok) != 0, np.uint8).reshape(-1)
        assert ob.shape == (n_obs,)
        obp = ob.ctypes.data_as(C.POINTER(C.c_uint8))
    R, t = np.array(R, np.float64, order="C").reshape(-1, 3, 3), np.array(t, np.float64, order="C").reshape(-1, 3)
    assert R.shape[0] == nc and t.shape[0] == nc
    q, tm, nu, st = np.empty((nc, 3)), np.zeros(3), np.empty(nc, np.int64), np.empty(nc, np.int32)
    raise_for(lib.mvba_pose_refine(_ptr(keep[0]), n, pp, cp, _ptr(xy), n_obs, m, okp, obp, _ptr(K), camp, nc, int(n_steps), _ptr(R), _ptr(t),
                                   _ptr(q), nu.ctypes.data_as(C.POINTER(C.c_int64)), st.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(tm),
                                   int(device)), lib)
    return {"R": R, "t": t, "quality": q, "n_usable": nu, "status": st, "timings_ms": dict(zip(("upload", "iterate", "other"), tm.tolist()))}


def pose_sample(seed, k, h, n):
    """The 4 distinct indices below ``n`` that hypothesis ``h`` of camera ``k`` draws (mvba_pose_sample: the host instance of
    the function the kernel runs; no GPU needed)."""
    return _sample("mvba_pose_sample", 4, seed, k, h, n)


def triangulate_robust(K, R, t, pt_ptr, cam_idx, xy, threshold, n_hypotheses=64, seed=0, n_refine=2, n_refit=2, return_counts=False,
                       device=-1):
    """Points by a two-view RANSAC per point on the device (mvba_triangulate_robust).  Cameras and list as for ``triangulate``;
    ``threshold`` is a reprojection distance in the units of xy.  Returns a dict: ``X (N, 3)``, ``quality (N, 3)`` (RMS
    reprojection residual, smallest depth and largest ray angle over the final inliers), ``status`` (N,) (0 ok, 1 fewer than two
    observations, 2 every hypothesis degenerate, 4 best count below min(deg, 3); X and quality NaN then), ``n_inliers``,
    ``best`` (N,), ``inlier (n_obs,) bool`` in the order of the list, ``hyp_count (N, H) int32`` (``return_counts``),
    ``timings_ms``.  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_triangulate_robust")
    K, R, t, xy = (_as(v, np.float64) for v in (K, R, t, xy))
    m, H = K.shape[0], int(n_hypotheses)
    assert K.shape == (m, 3, 3) and R.shape == (m, 3, 3) and t.shape == (m, 3)
    n, n_obs, pp, cp, xy = _obs_list(pt_ptr, cam_idx, xy, m)
    i32 = C.POINTER(C.c_int32)
    X, q, tm = np.empty((n, 3)), np.empty((n, 3)), np.zeros(4)
    st, ni, best, inl = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n_obs, np.uint8)
    hc = np.empty((n, max(H, 0)), np.int32) if return_counts else None
    raise_for(lib.mvba_triangulate_robust(_ptr(K), _ptr(R), _ptr(t), m, n, pp, cp, _ptr(xy), n_obs, float(threshold), H,
                                          _seed64(seed), int(n_refine), int(n_refit), _ptr(X), _ptr(q), st.ctypes.data_as(i32),
                                          ni.ctypes.data_as(i32), best.ctypes.data_as(i32), inl.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          hc.ctypes.data_as(i32) if return_counts else None, _ptr(tm), int(device)), lib)
    out = {"X": X, "quality": q, "status": st, "n_inliers": ni, "best": best, "inlier": inl.astype(bool),
           "timings_ms": dict(zip(("upload", "score", "refit", "download"), tm.tolist()))}
    if return_counts:
        out["hyp_count"] = hc
    return out


def triangulate_sample(seed, point, h, deg, n_hypotheses=64):
    """The two observation numbers (i < j, below ``deg``) of hypothesis ``h`` of point ``point``, or (-1, -1) where the
    exhaustive table has no entry ``h`` (mvba_triangulate_sample: the host instance of the function the kernel runs; no GPU
    needed)."""
    return _sample("mvba_triangulate_sample", 2, seed, point, h, deg, n_hypotheses)


def _align_args(src, dst, ok):
    """(src, dst, ok bytes or None, ok pointer, n) as mvba_align_robust and mvba_align take them."""
    src, dst = _as(src, np.float64), _as(dst, np.float64)
    n = src.shape[0]
    assert src.shape == (n, 3) and dst.shape == (n, 3)
    okb, okp = _point_ok_ptr(ok, n)
    return src, dst, okb, okp, n


def _similarity(sim):
    return {"s": float(sim[0]), "Q": sim[1:10].reshape(3, 3).copy(), "tau": sim[10:13].copy()}


def align_robust(src, dst, threshold, ok=None, with_scale=True, n_hypotheses=512, seed=0, n_refit=2, return_counts=False, device=-1):
    """The similarity ``dst ~ s Q src + tau`` by 3-point RANSAC on the device (mvba_align_robust).  ``src``, ``dst`` (n, 3); ``ok``
    (n,) marks the rows to use (rows with a non-finite number are unusable anyway); ``threshold`` is a distance in the units of
    dst.  Returns a dict: ``s``, ``Q (3, 3)``, ``tau (3,)``, ``quality (3,)`` (RMS residual over the final inliers, relative gap of
    the two largest eigenvalues of the last kept refit, mean squared spread of the inliers' src), ``n_usable``, ``n_inliers``,
    ``best``, ``status`` (0 ok, 1 fewer than 3 usable rows, 2 every hypothesis degenerate, 4 best count below 3; s, Q, tau and
    quality NaN then), ``inlier (n,) bool``, ``hyp_count (H,) int32`` (``return_counts``), ``timings_ms``.  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_align_robust")
    src, dst, okb, okp, n = _align_args(src, dst, ok)
    H = int(n_hypotheses)
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    sim, q, tm = np.empty(13), np.empty(3), np.zeros(4)
    nu, ni, best, st = C.c_int64(0), C.c_int64(0), C.c_int32(-1), C.c_int32(1)
    inl = np.empty(n, np.uint8)
    hc = np.empty(max(H, 0), np.int32) if return_counts else None
    raise_for(lib.mvba_align_robust(n, _ptr(src), _ptr(dst), okp, int(bool(with_scale)), float(threshold), H, _seed64(seed),
                                    int(n_refit), _ptr(sim), _ptr(q), C.byref(nu), C.byref(ni), C.byref(best), inl.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    None if hc is None else hc.ctypes.data_as(i32), C.byref(st), _ptr(tm), int(device)), lib)
    out = {**_similarity(sim), "quality": q, "n_usable": nu.value, "n_inliers": ni.value, "best": best.value, "status": st.value,
           "inlier": inl.astype(bool), "timings_ms": dict(zip(("upload", "score", "refit", "other"), tm.tolist()))}
    if hc is not None:
        out["hyp_count"] = hc
    return out


def align(src, dst, ok=None, with_scale=True, device=-1):
    """The least-squares similarity ``dst ~ s Q src + tau`` of every usable row on the device (mvba_align).  Returns a dict: ``s``,
    ``Q``, ``tau``, ``quality (3,)`` (RMS residual, eigenvalue gap, mean squared spread of src), ``n_usable``, ``status`` (0 ok, 1
    fewer than 3 usable rows, 2 degenerate: src or dst on a line).  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_align")
    src, dst, okb, okp, n = _align_args(src, dst, ok)
    sim, q = np.empty(13), np.empty(3)
    nu, st = C.c_int64(0), C.c_int32(1)
    raise_for(lib.mvba_align(n, _ptr(src), _ptr(dst), okp, int(bool(with_scale)), _ptr(sim), _ptr(q), C.byref(nu), C.byref(st), int(device)), lib)
    return {**_similarity(sim), "quality": q, "n_usable": nu.value, "status": st.value}


def align_sample(seed, h, n):
    """The 3 distinct indices below ``n`` that hypothesis ``h`` draws (mvba_align_sample: the host instance of the function the
    kernel runs; no GPU needed)."""
    return _sample("mvba_align_sample", 3, seed, h, n)


TRACK_COUNTS = ("n_tracks", "n_obs", "n_components", "n_short", "n_conflicting", "n_conflicting_nodes", "n_oversize",
                "n_oversize_nodes", "n_singletons", "n_rounds")  # counts [10] of mvba_build_tracks, in its order


def build_tracks(kp_ptr, kp_xy, edges, edge_ok=None, min_length=2, device=-1):
    """Feature tracks from pairwise matches on the device (mvba_build_tracks).  ``kp_ptr (m + 1,)``: keypoint j of image i is node
    ``kp_ptr[i] + j``; ``kp_xy (n_nodes, 2)`` or None; ``edges (E, 2)`` node ids; ``edge_ok (E,)`` marks the edges to use.
    Returns a dict: ``pt_ptr (T + 1,) int64``, ``cam_idx (n_obs,) int32``, ``obs_node (n_obs,) int32``, ``xy (n_obs, 2)`` (None
    without kp_xy), ``node_track (n_nodes,) int32`` (>= 0 the track, -1 unmatched, -2 too short, -3 conflicting or oversize), the
    ``TRACK_COUNTS`` by name, ``timings_ms``.  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_build_tracks")
    i32, i64, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    kp_ptr, edges = _as(kp_ptr, np.int64), _as(edges, np.int32).reshape(-1, 2)
    m, E = kp_ptr.shape[0] - 1, edges.shape[0]
    n = int(kp_ptr[-1]) if 0 <= int(kp_ptr[-1]) < 2 ** 31 else 0  # (a bad kp_ptr is refused before anything is written)
    kxp = okb = okp = None
    if kp_xy is not None:
        kp_xy = _as(kp_xy, np.float64).reshape(-1, 2)
        assert kp_xy.shape[0] == kp_ptr[-1]
        kxp = _ptr(kp_xy)
    if edge_ok is not None:
        okb = _as(np.asarray(edge_ok) != 0, np.uint8)
        assert okb.shape == (E,)
        okp = okb.ctypes.data_as(u8)
    pt_ptr, cam, node = np.empty(n // 2 + 1, np.int64), np.empty(n, np.int32), np.empty(n, np.int32)
    xy = None if kp_xy is None else np.empty((n, 2))
    track, counts, tm = np.empty(n, np.int32), np.zeros(len(TRACK_COUNTS), np.int64), np.zeros(4)
    raise_for(lib.mvba_build_tracks(m, kp_ptr.ctypes.data_as(i64), kxp, edges.ctypes.data_as(i32), E, okp, int(min_length),
                                    pt_ptr.ctypes.data_as(i64), cam.ctypes.data_as(i32), node.ctypes.data_as(i32),
                                    None if xy is None else _ptr(xy), track.ctypes.data_as(i32), counts.ctypes.data_as(i64), _ptr(tm),
                                    int(device)), lib)
    T, n_obs = int(counts[0]), int(counts[1])
    # (views of the buffers sized by n_nodes: the pages behind them that the call never wrote were never touched)
    return {"pt_ptr": pt_ptr[:T + 1], "cam_idx": cam[:n_obs], "obs_node": node[:n_obs], "xy": None if xy is None else xy[:n_obs], "node_track": track, **dict(zip(TRACK_COUNTS, counts.tolist())),
            "timings_ms": dict(zip(("upload", "labels", "layout", "download"), tm.tolist()))}


MATCH_COUNTS = ("n_matches", "n_queries", "n_no_candidate", "n_far", "n_ambiguous", "n_not_mutual")  # counts [6] of mvba_match_descriptors


def match_descriptors(kp_ptr, desc, pairs, ratio=0.0, mutual=True, max_dist2=-1, want_nn=False, device=-1):
    """Nearest-neighbour matching of uint8 descriptors on the device (mvba_match_descriptors).  ``kp_ptr (m + 1,)``: keypoint j of
    image i is row ``kp_ptr[i] + j`` of ``desc (n_nodes, dim) uint8``; ``pairs (P, 2)``: (query image, candidate image); ``ratio`` in
    (0, 1], 0 for no ratio test; ``max_dist2 < 0`` for no distance test.  Returns a dict: ``match_ptr (P + 1,) int64``,
    ``kp_pairs (M, 2) int32`` (keypoints local to their images), ``dist2 (M,) int32``, with ``want_nn`` the per-query ``nn_best``,
    ``nn_dist2``, ``nn_second2 (Q,) int32``, the ``MATCH_COUNTS`` by name, ``timings_ms``.  No CPU fallback."""
    lib = load_library()
    _require_device("mvba_match_descriptors")
    i32, i64, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    desc = np.asarray(desc)
    if desc.dtype != np.uint8 or desc.ndim != 2:
        raise ValueError(f"match_descriptors: desc must be (n_nodes, dim) uint8, got {desc.dtype} {desc.shape}")
    kp_ptr, desc, pairs = _as(kp_ptr, np.int64), _as(desc, np.uint8), _as(pairs, np.int32).reshape(-1, 2)
    m, P, dim = kp_ptr.shape[0] - 1, pairs.shape[0], desc.shape[1]
    assert m < 1 or desc.shape[0] == kp_ptr[-1]
    count = np.diff(kp_ptr)
    ok = m >= 1 and P > 0 and (count >= 0).all() and (pairs >= 0).all() and (pairs < m).all()
    Q = int(count[pairs[:, 0]].sum()) if ok else 0  # (bad arguments are refused before anything is written)
    Q = Q if Q < 2 ** 31 else 0
    match_ptr, kp_pairs, dist2 = np.zeros(P + 1, np.int64), np.empty((Q, 2), np.int32), np.empty(Q, np.int32)
    nn = [np.empty(Q, np.int32) for _ in range(3)] if want_nn else [None] * 3
    counts, tm = np.zeros(len(MATCH_COUNTS), np.int64), np.zeros(4)
    raise_for(lib.mvba_match_descriptors(m, kp_ptr.ctypes.data_as(i64), desc.ctypes.data_as(u8), dim, pairs.ctypes.data_as(i32), P,
                                         float(ratio), int(bool(mutual)), int(max_dist2), match_ptr.ctypes.data_as(i64),
                                         kp_pairs.ctypes.data_as(i32), dist2.ctypes.data_as(i32),
                                         *(None if a is None else a.ctypes.data_as(i32) for a in nn), counts.ctypes.data_as(i64), _ptr(tm),
                                         int(device)), lib)
    M = int(counts[0])
    out = {"match_ptr": match_ptr, "kp_pairs": kp_pairs[:M], "dist2": dist2[:M], **dict(zip(MATCH_COUNTS, counts.tolist())),
           "timings_ms": dict(zip(("upload", "distances", "tests", "download"), tm.tolist()))}
    if want_nn:
        out.update(zip(("nn_best", "nn_dist2", "nn_second2"), nn))
    return out


def host_obs_math(X3, cam15, xy2, f0):
    lib = load_library()
    out = np.empty(26)
    X3, cam15, xy2 = _as(X3, np.float64), _as(cam15, np.float64), _as(xy2, np.float64)
    raise_for(lib.mvba_host_obs_math(_ptr(X3), _ptr(cam15), _ptr(xy2), float(f0), _ptr(out)), lib)
    return out[:2], out[2:8].reshape(2, 3), out[8:].reshape(2, 9)


def _tm(tm):
    return {"h2d_ms": tm[0], "gram_ms": tm[1], "jacobi_ms": tm[2], "project_ms": tm[3], "sweeps": int(tm[4]),
            "refine_ms": tm[5]}


class SvdWorkspace:
    """Device-resident factorization workspace (mvsvd_create / load / run / destroy): buffers,
    stream and events are made once; ``load`` is the only host-to-device copy; ``run`` may be
    called any number of times on the resident matrix."""

    def __init__(self, max_rows, n_cols, dtype, device=-1):
        self.lib = load_library()
        if device_count() < 1:
            raise RuntimeError("libmvba: no HIP device visible; the SVD kernel has no CPU fallback")
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.float32, np.float64):
            raise ValueError("dtype must be float32 or float64")
        self.max_rows, self.n_cols, self.n_rows, self.base_rows = int(max_rows), int(n_cols), 0, 0
        h = C.c_void_p()
        raise_for(self.lib.mvsvd_create(self.max_rows, self.n_cols, 0 if self.dtype == np.float32 else 1, int(device),
                                        C.byref(h)), self.lib)
        self._h = h

    def load(self, Wt):
        Wt = np.ascontiguousarray(Wt, dtype=self.dtype)
        if Wt.ndim != 2 or Wt.shape[1] != self.n_cols:
            raise ValueError("Wt must be (n_rows, n_cols) of the workspace")
        raise_for(self.lib.mvsvd_load(self._h, Wt.ctypes.data, Wt.shape[0]), self.lib)
        self.n_rows = Wt.shape[0]
        return self

    def load_images(self, x_list):
        """The matrix np.hstack(x_list) (n_rows, 2 m) put together on the device from the images' (n_rows, 2) arrays themselves
        (all float32 or all float64; converted to the workspace's dtype)."""
        src = np.result_type(*x_list)
        if src not in (np.float32, np.float64):
            raise ValueError("image arrays must be float32 or float64")
        arrs = [np.ascontiguousarray(a, dtype=src) for a in x_list]
        n_rows = arrs[0].shape[0]
        if 2 * len(arrs) != self.n_cols or any(a.shape != (n_rows, 2) for a in arrs):
            raise ValueError("x_list must hold n_cols / 2 arrays of shape (n_rows, 2)")
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        raise_for(self.lib.mvsvd_load_images(self._h, ptrs, len(arrs), n_rows, 0 if src == np.float32 else 1), self.lib)
        self.n_rows = n_rows
        return self

    def load_base(self, X):
        """The resident base matrix of run_scaled (one upload for a whole depth loop)."""
        X = np.ascontiguousarray(X, dtype=self.dtype)
        if X.ndim != 2 or X.shape[1] != self.n_cols:
            raise ValueError("X must be (n_rows, n_cols) of the workspace")
        raise_for(self.lib.mvsvd_load_base(self._h, X.ctypes.data, X.shape[0]), self.lib)
        self.base_rows = X.shape[0]
        return self

    def load_base_images(self, x_list, f0):
        """The base (x / f0, y / f0, 1) per image, assembled on the device from the images' (n_rows, 2) arrays themselves."""
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in x_list]
        n_rows = arrs[0].shape[0]
        if 3 * len(arrs) != self.n_cols or any(a.shape != (n_rows, 2) for a in arrs):
            raise ValueError("x_list must hold n_cols / 3 arrays of shape (n_rows, 2)")
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        raise_for(self.lib.mvsvd_load_base_images(self._h, ptrs, len(arrs), n_rows, float(f0)), self.lib)
        self.base_rows = n_rows
        return self

    def run_scaled(self, z, group, norm, n_rank):
        """Factorise X o z (depths z (n_rows, n_cols / group) per column group, normalised: norm 1 = unit rows,
        2 = column groups by their squared norm) from the resident base: only z is uploaded.
        M (n_cols, r), sigma (n_cols,), S (r, n_rows), timings.  z = None: the depths a device depth loop left in the workspace."""
        if z is not None:
            z = np.ascontiguousarray(z, dtype=self.dtype)
            if z.shape != (self.base_rows, self.n_cols // int(group)):
                raise ValueError("z must be (rows of the base, n_cols / group)")
        self.n_rows = self.base_rows  # the workspace matrix becomes the re-weighted base
        M = np.empty((self.n_cols, n_rank), self.dtype)
        sigma = np.empty(self.n_cols, self.dtype)
        S = np.empty((n_rank, self.n_rows), self.dtype)
        tm = np.zeros(6)
        raise_for(self.lib.mvsvd_run_scaled(self._h, z.ctypes.data if z is not None else None, int(group), int(norm), int(n_rank), M.ctypes.data,
                                            sigma.ctypes.data, S.ctypes.data, _ptr(tm)), self.lib)
        return M, sigma, S, _tm(tm)

    # -- the projective-depth loops on the device (ref perspective_camera_calibration.py:61-144, :147-235)
    def depth_begin(self, group=3):
        """z <- 1 on the device for the resident base (homogeneous image coordinates: group = 3)."""
        raise_for(self.lib.mvsvd_depth_begin(self._h, int(group)), self.lib)

    def depth_step(self, method, f0):
        """One iteration (1 = primary, 2 = dual): re-weight, factorise, update the depths on the device.
        Returns (reprojection error, timings); nothing else crosses PCIe."""
        E = C.c_double()
        tm = np.zeros(6)
        raise_for(self.lib.mvsvd_depth_step(self._h, int(method), float(f0), C.byref(E), _ptr(tm)), self.lib)
        t = _tm(tm)
        t["depth_ms"] = t.pop("h2d_ms")  # (slot 0 of a depth step: the depth-update kernels)
        return E.value, t

    def depth_read(self):
        """The current depths (rows of the base, n_cols / 3), float64."""
        z = np.empty((self.base_rows, self.n_cols // 3), self.dtype)
        raise_for(self.lib.mvsvd_depth_read(self._h, z.ctypes.data), self.lib)
        return z.astype(np.float64, copy=False)

    def run(self, n_rank, center=False):
        """M (n_cols, r), sigma (n_cols,), S (r, n_rows), means (n_cols,), timings."""
        M = np.empty((self.n_cols, n_rank), self.dtype)
        sigma = np.empty(self.n_cols, self.dtype)
        S = np.empty((n_rank, self.n_rows), self.dtype)
        means = np.zeros(self.n_cols, self.dtype)
        tm = np.zeros(6)
        raise_for(self.lib.mvsvd_run(self._h, int(n_rank), int(bool(center)), M.ctypes.data, sigma.ctypes.data,
                                     S.ctypes.data, means.ctypes.data, _ptr(tm)), self.lib)
        return M, sigma, S, means, _tm(tm)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mvsvd_destroy(self._h)
            self._h = None

    __del__ = close


_svd_cache = {}  # (dtype, n_cols, device) -> SvdWorkspace kept between public factorization calls
_svd_cache_lock = threading.Lock()  # (ranks may be threads of one process: lib._distributed.InProcessGroup)
_svd_cache_atexit = False


def _svd_cache_clear():
    """Release the cached SVD workspaces (~2 GB of device memory at config 5); also registered at interpreter exit."""
    with _svd_cache_lock:
        for ws in _svd_cache.values():
            ws.close()
        _svd_cache.clear()


svd_cache_clear = _svd_cache_clear  # public name: call it to hand the cached workspaces' device memory back (e.g. before a large BundleAdjuster)


def _svd_cache_usable(n_rows, n_cols, n_rank):
    return os.environ.get("MVBA_SVD_CACHE", "1") != "0" and n_rows >= 1 and 1 <= n_rank <= n_cols <= 12288


def _svd_cached_run(dtype, n_rows, n_cols, device, load, n_rank, center):
    """`load(ws)` then `ws.run(n_rank, center)` on the cached workspace of (dtype, n_cols, device), made or grown as needed."""
    global _svd_cache_atexit
    dtype = np.dtype(dtype)
    key = (dtype.str, n_cols, int(device))
    with _svd_cache_lock:  # (held through the call: a workspace is one matrix and one stream)
        ws = _svd_cache.get(key)
        if ws is None or ws.max_rows < n_rows:
            old = _svd_cache.pop(key, None)  # out of the cache BEFORE it is closed: a failing allocation below must not leave a closed handle behind
            if old is not None:
                old.close()
            if not _svd_cache_atexit:
                import atexit

                atexit.register(_svd_cache_clear)
                _svd_cache_atexit = True
            ws = SvdWorkspace(n_rows, n_cols, dtype, device)
            _svd_cache[key] = ws
        load(ws)
        return ws.run(n_rank, center)


def svd_factorize_images(x_list, n_rank, center=False, device=-1):
    """`svd_factorize(np.hstack(x_list), ...)` without the hstack: the images' (n_rows, 2) arrays (all float32 or all float64) go to
    the device as they are and the (n_rows, 2 m) matrix is put together there (`mvsvd_load_images`).  Anything else -- other
    dtypes, ragged lists, the cache switched off -- takes the host's hstack."""
    if device_count() < 1:
        raise RuntimeError("libmvba: no HIP device visible; the SVD kernel has no CPU fallback")
    arrs = [np.asarray(a) for a in x_list]
    n_rows, n_cols = (arrs[0].shape[0] if arrs and arrs[0].ndim == 2 else 0), 2 * len(arrs)
    dt = np.result_type(*arrs) if arrs else np.dtype(np.float64)
    if (dt in (np.float32, np.float64) and all(a.shape == (n_rows, 2) for a in arrs) and _svd_cache_usable(n_rows, n_cols, n_rank)):
        return _svd_cached_run(dt, n_rows, n_cols, device, lambda ws: ws.load_images(arrs), n_rank, center)
    return svd_factorize(np.ascontiguousarray(np.hstack(arrs)), n_rank, center, device)


def svd_factorize(Wt, n_rank, center=False, device=-1):
    """Thin SVD of W = Wt^T.  Wt: (n_rows, n_cols) float32/float64, C-contiguous.
    Returns M (n_cols, r), sigma (n_cols,), S (r, n_rows), means (n_cols,), timings.
    A workspace (device buffers, stream, events: `mvsvd_create`) is KEPT between calls per (dtype, n_cols, device) and grown
    when a larger matrix arrives -- at config 5 allocating and freeing ~1 GB of device memory per call cost more than the
    PCIe copy of the matrix; `MVBA_SVD_CACHE=0` restores the one-shot `mvsvd_factorize` (create + load + run + destroy),
    `_svd_cache_clear()` (also at interpreter exit) releases the memory."""
    lib = load_library()
    if device_count() < 1:
        raise RuntimeError("libmvba: no HIP device visible; the SVD kernel has no CPU fallback")
    Wt = np.ascontiguousarray(Wt)
    if Wt.dtype not in (np.float32, np.float64):
        Wt = Wt.astype(np.float64)
    n_rows, n_cols = Wt.shape
    if _svd_cache_usable(n_rows, n_cols, n_rank):
        return _svd_cached_run(Wt.dtype, n_rows, n_cols, device, lambda ws: ws.load(Wt), n_rank, center)
    M = np.empty((n_cols, n_rank), Wt.dtype)
    sigma = np.empty(n_cols, Wt.dtype)
    S = np.empty((n_rank, n_rows), Wt.dtype)
    means = np.zeros(n_cols, Wt.dtype)
    tm = np.zeros(6)
    rc = lib.mvsvd_factorize(Wt.ctypes.data, n_rows, n_cols, 0 if Wt.dtype == np.float32 else 1, int(n_rank),
                             int(bool(center)), M.ctypes.data, sigma.ctypes.data, S.ctypes.data, means.ctypes.data,
                             _ptr(tm), int(device))
    raise_for(rc, lib)
    return M, sigma, S, means, _tm(tm)
