"""Bundle-adjustment problems in pixel units (f0 != 1, f ~ f0, off-centre principal points) and their unit twins.
Test infrastructure only.

A pixel problem (xy_px, f0, f_px, u_px) and its unit twin (xy_px / f0, 1, f_px / f0, u_px / f0) with the same X, t, R are
the same problem.  With D the 9m-vector that holds f0 at the (f, u, v) slots of every camera and 1 at the pose slots:
residuals, J_X, E, dP, weights, costs, dX and the trial points are equal; JC_twin = JC_px D (column-wise);
A_twin = D A_px D, b_twin = D b_px; dxi_twin = dxi_px / D; f and u scale by 1 / f0; camera covariances by D_i D_j;
residuals() by f0.  With f0 a power of two every one of these factors is exact, so two engines that run the same
operations in the same order agree bit for bit after the scaling.

``assert_twin`` compares two dictionaries of such quantities (``engine_outputs`` fills one from any engine that speaks
the HipEngine protocol); ``exact=False`` uses the bounds of the existing test of each quantity (``TWIN_TOL``)."""
import numpy as np

from lib.bundle_adjustment import to_gauge_frame
from lib.synthetic import make_scene
from oracle import ba_oracle as O

PP_CENTRE = (320.0, 240.0)  # u != v: a swapped pair shows
MARGIN = 100  # the project's usual factor between a measured reference error and the bound set from it (tests/_init_cases.py)

# Where the ORACLE's own rounding at f0 = 600 exceeds the existing 1e-9 bound on dxi: max|dxi_px / D - dxi_twin| / max|dxi_twin|
# between the oracle on the pixel problem and the oracle on its twin, keyed by (shape, loss) -- measured and re-checked by
# tests/test_pixel_units_cpu.py::test_recorded_oracle_twin_differences.  The pixel system is unscaled (condition number 6.6e9
# against the twin's 1.5e5 at 90 x 70) and NumPy's LU of it loses that much; the device's Cholesky does not: its distance
# from the f0 = 600 oracle on these cases IS this figure (2.357e-9 and 1.442e-9 measured on both sides), i.e. it sits on the
# oracle's twin solve.  Against the f0 = 600 oracle the bound on dxi (and on the trial f, u, which are state + dxi) is
# MARGIN times the recorded figure on these cases and the existing one everywhere else.
ORACLE_TWIN_DXI = {
    ((3000, 647, 0.04), "squared"): 1.5e-9,  # measured 1.442e-9
    ((90, 70, 1.0), "squared"): 2.5e-9,      # measured 2.357e-9
    ((3000, 647, 0.04), "cauchy"): 1.5e-9,   # measured 1.39e-9 (huber on the same scene: 7.9e-10, within the existing bound)
}


def dxi_bound(shape, loss="squared", existing=1e-9):
    """The bound on dxi (fraction of max|dxi|, twin's units) against the f0 = 600 oracle on the case (shape, loss)."""
    return max(existing, MARGIN * ORACLE_TWIN_DXI.get((tuple(shape), loss), 0.0))


# How each quantity of the PIXEL problem goes to the twin's units.  Everything not named here is equal in both.
#   "JC"   (n_obs, 2, 9) * D[:9]        "A"  (9m, 9m) * D_i D_j     "b" (9m,) * D      "dxi" (9m,) / D
#   "trial_cam" (m, 15): columns f, u, v / f0                         "f" (m,), "u" (m, 2) / f0
#   "cov_cameras" (m, 9, 9) / (D_i D_j),  "cov_full" (9m, 9m) / (D_i D_j)          "residuals_px" (n_obs, 2) / f0

# exact=False: (rtol, atol as a fraction of max|twin|, absolute atol) -- the bounds of _parity_checks.check_one_step
# (cost, residual .. trial state), tests/test_gpu_robust.py::_check_step (weight) and tests/test_gpu_covariance.py (1e-8),
# each on the quantity in the twin's units.
TWIN_TOL = {
    "cost": (1e-13, 0.0, 0.0),
    "residual": (1e-12, 0.0, 1e-14),
    "JX": (1e-12, 0.0, 1e-13),
    "JC": (1e-12, 0.0, 1e-12),
    "weight": (0.0, 1e-12, 0.0),
    "E": (1e-11, 1e-12, 0.0),
    "dP": (1e-11, 1e-12, 0.0),  # (of max|dP|: the caller's sum-of-terms scale is not in the dictionary; this is tighter)
    "A": (0.0, 1e-12, 0.0),
    "b": (0.0, 1e-10, 0.0),
    "dxi": (0.0, 1e-9, 0.0),
    "dX": (0.0, 1e-9, 0.0),
    "trial_X": (0.0, 0.0, 1e-10),
    "trial_cam": (0.0, 0.0, 1e-10),
    "trial_cost": (1e-9, 0.0, 1e-13),
    "residuals_px": (1e-12, 0.0, 1e-14),
    "cov_points": (0.0, 1e-8, 0.0),
    "cov_cameras": (0.0, 1e-8, 0.0),
    "cov_full": (0.0, 1e-8, 0.0),
    "X": (0.0, 0.0, 1e-9), "f": (0.0, 0.0, 1e-9), "u": (0.0, 0.0, 1e-9), "t": (0.0, 0.0, 1e-9), "R": (0.0, 0.0, 1e-9),
}


def scale_vector(m, f0):
    """D (9m,): f0 at (f, u, v) of every camera, 1 at t and omega."""
    D = np.ones((m, 9))
    D[:, :3] = f0
    return D.reshape(-1)


def pixel_problem(n, m, p, f0, pp_seed=17, outlier_frac=0.0, one_body=False, **scene_kw):
    """(px_prob, twin_prob, D): the 12-tuples (n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R) of the GPU tests for the
    make_scene(n, m, vis_p=p) scene in pixel units and for its unit twin, and the scale vector D.

    The pixel inputs come first -- f_px = f0 init_f, u_px = (320, 240) + N(0, 5) per camera, xy_px = f0 xy + u_true[cam]
    with u_true = u_px + N(0, 1.5) so that the gradient in u is not zero -- and the twin is those very arrays divided
    by f0.  ``outlier_frac``: that share of the observations displaced by 20-100 px (for the robust losses);
    ``one_body``: every camera starts from the mean f and one u (what a shared-intrinsics map requires)."""
    sc = make_scene(n, m, vis_p=p, project="numpy", **scene_kw)
    X, R, t = to_gauge_frame(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    rng = np.random.default_rng(pp_seed)
    u_px = np.array(PP_CENTRE) + rng.normal(0.0, 5.0, (m, 2))
    u_true = u_px + rng.normal(0.0, 1.5, (m, 2))
    f_px = f0 * sc.init_K[:, 0, 0]
    xy_px = f0 * sc.xy + u_true[sc.cam_idx]
    if outlier_frac:
        idx = rng.choice(len(xy_px), size=max(1, int(round(outlier_frac * len(xy_px)))), replace=False)
        ang, r = rng.uniform(0.0, 2.0 * np.pi, idx.size), rng.uniform(20.0, 100.0, idx.size)
        xy_px[idx] += np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    if one_body:
        f_px = np.full(m, f_px.mean())
        u_px = np.tile(u_px.mean(axis=0), (m, 1))
    f0 = float(f0)
    px = (n, m, sc.pt_ptr, sc.cam_idx, xy_px, f0, sc.axis, X, f_px, u_px, t, R)
    twin = (n, m, sc.pt_ptr, sc.cam_idx, xy_px / f0, 1.0, sc.axis, X, f_px / f0, u_px / f0, t, R)
    return px, twin, scale_vector(m, f0)


def to_twin_units(key, v, D):
    """The pixel problem's quantity ``key`` in the twin's units (exact when f0 is a power of two)."""
    v = np.asarray(v, np.float64)
    f0 = D[0]
    if key == "JC":
        return v * D[:9]
    if key in ("A", "cov_full"):
        DD = np.outer(D, D)
        return v.reshape(len(D), len(D)) * DD if key == "A" else v / DD
    if key == "cov_cameras":
        return v / np.outer(D[:9], D[:9])
    if key == "b":
        return v * D
    if key == "dxi":
        return v / D
    if key == "trial_cam":
        out = v.copy()
        out[:, :3] /= f0
        return out
    if key in ("f", "u", "residuals_px"):
        return v / f0
    return v


def assert_twin(px_out, twin_out, D, exact):
    """Every quantity of ``px_out`` (pixel problem) against ``twin_out`` (unit twin) after scaling to the twin's units:
    bit for bit when ``exact``, else within TWIN_TOL.  Integers (``n_solves``, ``lu_fallback``) are always compared as
    they are.  Prints the largest difference of each quantity beside its bound; returns them as a dictionary."""
    assert set(px_out) == set(twin_out)
    worst = {}
    for key in px_out:
        a, b = px_out[key], twin_out[key]
        if isinstance(a, (int, np.integer)):
            assert a == b, (key, a, b)
            continue
        b = np.asarray(b, np.float64)
        if key == "A":
            b = b.reshape(len(D), len(D))
        a = to_twin_units(key, a, D)
        assert a.shape == b.shape, (key, a.shape, b.shape)
        assert np.isfinite(a).all() and np.isfinite(b).all(), key
        diff = float(np.abs(a - b).max()) if a.size else 0.0
        scale = float(np.abs(b).max()) if b.size else 0.0
        worst[key] = diff / scale if scale else diff
        if exact:
            print(f"  twin {key}: max|diff| / max = {worst[key]:.3e} (bound: bitwise)")
            assert np.array_equal(a, b), (key, diff, scale)
        else:
            rtol, frac, atol = TWIN_TOL[key]
            print(f"  twin {key}: max|diff| / max = {worst[key]:.3e} (bound: rtol {rtol:g}, atol {frac:g} max + {atol:g})")
            np.testing.assert_allclose(a, b, rtol=rtol, atol=frac * scale + atol, err_msg=key)
    return worst


def make_engine(cls, prob, **kw):
    """``cls`` (HipEngine or an oracle engine) on the 12-tuple ``prob``, state set."""
    n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R = prob
    eng = cls(n, m, pt_ptr, cam, xy, f0, axis, **kw)
    eng.set_params(X, f, u, t, R)
    return eng


def engine_outputs(eng, c, keys=None):
    """cost, one linearisation and one trial at damping ``c`` of an engine at its committed state, as the dictionary
    assert_twin takes.  A HipEngine is read through debug_read / residuals(); an oracle engine through its attributes.
    ``keys``: keep only these."""
    out = {"cost": eng.cost()}
    eng.linearize()
    if hasattr(eng, "debug_read"):
        m, n_obs = eng.m, eng.n_obs
        out["residual"] = eng.debug_read("residual").reshape(n_obs, 2)
        out["JX"] = eng.debug_read("JX").reshape(n_obs, 2, 3)
        out["JC"] = eng.debug_read("JC").reshape(n_obs, 2, 9)
        out["E"] = eng.debug_read("E").reshape(-1, 6)
        out["dP"] = eng.debug_read("dP").reshape(-1, 3)
        if eng.loss != "squared":
            out["weight"] = eng.debug_read("weight")
        out["trial_cost"] = eng.try_step(c)
        out["A"] = eng.debug_read("A_full").reshape(9 * m, 9 * m)
        out["b"] = eng.debug_read("b_full")
        out["dxi"] = eng.debug_read("dxi")
        out["dX"] = eng.debug_read("dX").reshape(-1, 3)
        out["trial_X"] = eng.debug_read("trial_X").reshape(-1, 3)
        out["trial_cam"] = eng.debug_read("trial_cam").reshape(m, 15)
        out["residuals_px"] = eng.residuals()
    else:
        m = eng.m
        iu = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])
        out.update(residual=eng.e, JX=eng.JX, JC=eng.JC, E=eng.E[:, iu[0], iu[1]], dP=eng.dP)
        if hasattr(eng, "w"):
            out["weight"] = np.sqrt(eng.w)
        A, b = eng.reduced_system(c)  # (try_step of a single-rank oracle, with the full-length increment kept)
        out["A"], out["b"] = A, b
        out["dxi"] = np.array(eng.solve_reduced(A, b))
        out["trial_cost"] = eng.apply_step(out["dxi"])
        out["dX"] = eng.dX
        out["trial_X"] = eng.tX
        out["trial_cam"] = np.concatenate([eng.tf[:, None], eng.tu, eng.tt, eng.tR.reshape(m, 9)], axis=1)
        out["residuals_px"] = eng.f0 * O.residuals(eng.X, eng.f, eng.u, eng.t, eng.R, eng.f0, eng.pt, eng.cam, eng.xy)
    if keys is not None:
        out = {k: out[k] for k in keys}
    return out
