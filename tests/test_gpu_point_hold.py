"""Held points on the HIP engine (mvba_set_point_hold) against the references of tests/_point_hold_ref.py:
one step under every kind of mask, every Schur form and the block edges of K3a, legal degeneracy, the invariants, whole
trajectories, camera refinement against known structure, covariances and the C ABI.  Tolerances are those of the existing
test of the same quantity (tests/test_gpu_constraints.py::_check_step, tests/test_gpu_parity.py,
tests/test_gpu_covariance.py); each is named at its assert."""
import ctypes as C

import numpy as np
import pytest

import _pose_ransac_ref as PR
from _point_hold_ref import HeldOracleEngine, HeldRefAdjuster, HeldRobustEngine, dense_covariance_held, masks
from lib import _mvba
from lib.bundle_adjustment import AXES, BundleAdjuster, lm_loop, parameter_map, residual_variance
from lib.initialization import refine_poses
from lib.synthetic import make_scene
from oracle import ba_oracle as O
from test_gpu_constraints import ROUTES, _check_step, _golden_problem, _scene_problem

pytestmark = pytest.mark.gpu


def _pair(n, m, pt_ptr, cam, xy, axis, state, **kw):
    eng = _mvba.HipEngine(n, m, pt_ptr, cam, xy, 1.0, axis, **kw)
    ref = (HeldRobustEngine if kw else HeldOracleEngine)(n, m, pt_ptr, cam, np.asarray(xy).reshape(-1, 2), 1.0, axis, **kw)
    eng.set_params(*state)
    ref.set_params(*state)
    return eng, ref


def _hold(eng, ref, mask, col, n_free):
    for e in (eng, ref):
        e.set_parameter_map(col, n_free)
        e.set_point_hold(mask)
    assert eng.n_held_points == ref.n_held_points == int(mask.sum())


def _check_held_step(eng, ref, mask, col, n_free, c, X, **tol):
    """_check_step (tests/test_gpu_constraints.py: dxi 1e-9 of max|dxi|, dX 1e-9 of max|dX|, trial state 1e-10, trial cost
    1e-12) and, exactly: no step and no move at held points."""
    E = _check_step(eng, ref, col, n_free, c, **tol)
    dX, tX = eng.debug_read("dX").reshape(-1, 3), eng.debug_read("trial_X").reshape(-1, 3)
    assert (dX[mask] == 0).all() and np.array_equal(tX[mask], X[mask])
    assert mask.all() or (dX[~mask] != 0).any()
    return E


# ---------------------------------------------------------------- 1: one step against the reference
@pytest.mark.parametrize("scene", ["linearize_60x7_xup", "linearize_60x7_xright", "2000x30"])
def test_one_step_for_every_kind_of_mask(golden, scene):
    if scene == "2000x30":
        prob = _scene_problem(2000, 30, 0.3)
    else:
        prob = _golden_problem(golden(scene), "x-up_z-forward" if scene.endswith("xup") else "x-right_z-forward")
    n, m, pt_ptr, cam, xy, axis, state = prob
    eng, ref = _pair(*prob)
    eng.linearize()
    ref.linearize()
    E6, dP = eng.debug_read("E"), eng.debug_read("dP")
    for name, mask in masks(n).items():
        col, n_free = parameter_map(m, axis, hold="intrinsics") if name == "random40" else parameter_map(m, axis)
        _hold(eng, ref, mask, col, n_free)  # (keeps the linearisation)
        for c in (1e-4, 1e-1):
            print(scene, name, end=" ")
            _check_held_step(eng, ref, mask, col, n_free, c, state[0])
        assert np.array_equal(eng.debug_read("E"), E6) and np.array_equal(eng.debug_read("dP"), dP)  # the undamped sums stay
    assert eng.stats()["counts"]["lu_fallback"] == 0


# ---------------------------------------------------------------- 2: every Schur form, the block edges of K3a
# (ROUTES has a lanes row of its own, at 3000 x 14 x 0.5; this file keeps its row, at the shape of tests/test_gpu_schur_lanes.py)
FORMS = [r for r in ROUTES if r[0] != "lanes"] + [("lanes", (3000, 12, 0.5), {"MVBA_SCHUR": "lanes"})]


@pytest.mark.parametrize("route,shape,env", FORMS, ids=[r[0] for r in FORMS])
def test_every_schur_form_and_the_block_edges(route, shape, env, monkeypatch):
    """k_point_inv moves 256 points per block through LDS: the mask holds points 0, 255, 256 and N - 1 (3001 is no multiple
    of 256) and every fifth point.  Bounds and route checks as tests/test_gpu_constraints.py::test_every_route_into_the_solve."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = _scene_problem(*shape)
    n, m, pt_ptr, cam, xy, axis, state = prob
    eng, ref = _pair(*prob)
    if route in ("pairs", "slots", "dense"):
        assert eng.schur_info()["kernel"] == route
    if route == "lanes":  # as tests/test_gpu_schur_lanes.py::_took
        info = eng.schur_info()
        assert info["kernel"] == "slots" and info["step_width"] == 64, info
    mask = np.arange(n) % 5 == 2
    mask[[0, 255, 256, n - 1]] = True
    col, n_free = parameter_map(m, axis)
    _hold(eng, ref, mask, col, n_free)
    eng.linearize()
    ref.linearize()
    print(route, end=" ")
    if route == "gcam647":  # the bounds of test_extreme_camera_counts_vs_oracle: dxi 1e-7, cost 1e-7
        _check_held_step(eng, ref, mask, col, n_free, 1e-2, state[0], dxi_tol=1e-7, e_tol=1e-7, dx_tol=1e-7, trial_tol=1e-7)
    else:
        _check_held_step(eng, ref, mask, col, n_free, 1e-4, state[0])
    # the neighbours of the held points at a block edge are free points like any other (their rows are not disturbed)
    dX = eng.debug_read("dX").reshape(-1, 3)
    assert (dX[[1, 254, 258, n - 2]] != 0).all()
    st = eng.stats()["counts"]
    assert st["lu_fallback"] == 0
    if route == "polls0":
        assert st["barrier_fallback"] == (1 if n_free > 128 else 0)


# ---------------------------------------------------------------- 3: legal degeneracy
def test_a_held_point_seen_once_is_legal_a_free_one_is_not():
    sc = make_scene(300, 6, vis_p=0.7)
    once = np.array([0, 17, 255, 256, 299])
    keep = np.ones(len(sc.cam_idx), bool)
    for a in once:  # these keep their first observation only
        keep[sc.pt_ptr[a] + 1:sc.pt_ptr[a + 1]] = False
    pt_ptr = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(np.int64), sc.pt_ptr[:-1]))])
    cam, xy = sc.cam_idx[keep], sc.xy[keep]
    assert (np.diff(pt_ptr)[once] == 1).all()
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    state = (X, sc.init_K[:, 0, 0].copy(), sc.init_K[:, :2, 2].copy(), t, R)
    eng, ref = _pair(sc.n_points, 6, pt_ptr, cam, xy, sc.axis, state)
    with pytest.raises(np.linalg.LinAlgError, match="point block"):  # free: as today (the same scene, the same engine)
        eng.covariance()
    mask = np.zeros(sc.n_points, bool)
    mask[once] = True
    col, n_free = parameter_map(6, sc.axis)
    _hold(eng, ref, mask, col, n_free)
    eng.linearize()
    ref.linearize()
    _check_held_step(eng, ref, mask, col, n_free, 1e-4, X)
    cov = eng.covariance(full=True)
    assert not cov["points"][mask].any() and np.isfinite(cov["points"]).all() and (cov["points"][~mask][:, [0, 1, 2], [0, 1, 2]] > 0).all()
    want = dense_covariance_held(sc.n_points, 6, pt_ptr, cam, xy, 1.0, col, n_free, mask, *state)
    for k in ("points", "cameras", "cameras_full"):  # DESIGN.md §11's bound, as tests/test_gpu_constraints.py::test_covariance_under_a_map
        err = np.abs(cov[k] - want[k]).max() / np.abs(want[k]).max()
        print(k, f"max err / max entry = {err:.3e}")
        assert err <= 1e-8, k
    eng.set_point_hold(None)
    with pytest.raises(np.linalg.LinAlgError, match="point block"):
        eng.covariance()


# ---------------------------------------------------------------- 4: invariants
def _step_record(eng, c=1e-4):
    E = eng.try_step(c)
    return E, eng.debug_read("A_full"), eng.debug_read("b_full"), eng.debug_read("dxi"), eng.debug_read("dX")


def test_set_then_clear_is_the_engine_that_never_had_a_mask_and_runs_repeat_bitwise():
    prob = _scene_problem(2000, 30, 0.3)
    n = prob[0]
    mask = masks(n)["random40"]
    out = {}
    for how in ("never", "cleared", "empty", "held", "held_again"):
        eng, _ = _pair(*prob)
        eng.linearize()
        if how in ("cleared", "empty"):
            eng.set_point_hold(mask)
            eng.try_step(1e-4)
            eng.set_point_hold(None if how == "cleared" else np.zeros(n, bool))
            assert eng.n_held_points == 0
        if how.startswith("held"):
            eng.set_point_hold(mask)
        out[how] = _step_record(eng)
    for how in ("cleared", "empty"):
        for a, b in zip(out["never"], out[how]):
            assert np.array_equal(a, b), how
    for a, b in zip(out["held"], out["held_again"]):
        assert np.array_equal(a, b)
    assert not np.array_equal(out["held"][1], out["never"][1]) and out["held"][0] != out["never"][0]


def test_everything_held_moves_nothing():
    prob = _scene_problem(2000, 30, 0.3)
    n, m, axis, state = prob[0], prob[1], prob[5], prob[6]
    eng, _ = _pair(*prob)
    col, n_free = parameter_map(m, axis, hold="cameras")
    assert n_free == 0
    eng.set_parameter_map(col, n_free)
    eng.set_point_hold(np.ones(n, bool))
    E0 = eng.cost()
    eng.linearize()
    for c in (1e-4, 1e-1):
        assert eng.try_step(c) == E0
        assert np.array_equal(eng.debug_read("trial_X").reshape(-1, 3), state[0])
        assert not eng.debug_read("dX").any() and not eng.debug_read("dxi").any()
    eng.commit()
    for a, b in zip(eng.get_params(), state):
        assert np.array_equal(a, b)
    assert eng.cost() == E0


# ---------------------------------------------------------------- 5: trajectories
def _euclid_inputs(golden, outliers):
    d = golden("euclid_default")
    x = np.array(d["x"], np.float64, copy=True)
    if outliers:  # the recipe of tests/test_gpu_constraints.py::test_huber_trajectory_with_held_intrinsics, in this scene's units
        live = np.argwhere(np.ones(x.shape[:2], bool))
        rng = np.random.default_rng(11)
        pick = live[rng.choice(len(live), size=max(1, len(live) // 15), replace=False)]
        ang = rng.uniform(0, 2 * np.pi, len(pick))
        r = rng.uniform(0.05, 0.3, len(pick))
        x[pick[:, 0], pick[:, 1]] += np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    return d, x


@pytest.mark.parametrize("loss", ["squared", "huber"])
def test_trajectory_vs_reference(golden, loss):
    """euclid_default's inputs, every other point held at its initial value, the arguments of
    tests/test_gpu_parity.py::test_full_trajectory_vs_reference and its bounds: equal counts of iterations and solves, every
    logged cost 1e-9 relative, outputs 1e-9.  (The reference keeps its counts, 28 outer / 43 solves squared and 27 / 42 huber,
    when A is perturbed by 1e-13 relative: no accept test of these runs falls within rounding.)  huber: a fifteenth of the
    observations displaced by 0.05 .. 0.3, scale 0.01 -- 373 of 2000 observations end with a weight below 1."""
    d, x = _euclid_inputs(golden, loss == "huber")
    kw = dict(loss="huber", loss_scale=0.01) if loss == "huber" else {}
    half = np.arange(x.shape[0]) % 2 == 0
    out = []
    for cls in (BundleAdjuster, HeldRefAdjuster):
        ba = cls(x, d["init_X"], d["init_K"], d["init_R"], d["init_t"], axis="x-up_z-forward", hold_points=half, **kw)
        res = ba.optimize(2.0, 1e-8, 100, is_debug=True)
        out.append((res, np.array([e["reprojection_error"] for e in ba.get_log()]), ba._engine.n_solves))
        assert ba.n_held_points == half.sum() == ba._engine.n_held_points
    (got, E, ns), (want, Eo, nso) = out
    print(loss, "outer", len(E) - 1, len(Eo) - 1, "solves", ns, nso, "max rel dE", np.abs(E[:len(Eo)] / Eo[:len(E)] - 1).max())
    assert len(E) == len(Eo) and ns == nso
    np.testing.assert_allclose(E, Eo, rtol=1e-9, atol=1e-12)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
    assert np.array_equal(got[0][half], d["init_X"][half])  # bit for bit
    assert not np.array_equal(got[0][~half], d["init_X"][~half]) and E[-1] < E[0]


# ---------------------------------------------------------------- 6: camera refinement against known structure
def test_cameras_against_known_structure_reach_the_poses_of_refine_poses():
    """Ground-truth points all held, intrinsics held at the truth, camera 0 at its true pose, noisy poses for cameras >= 1:
    optimize() and refine_poses minimise the same cost, camera by camera, in the same unknowns -- except camera 1's translation
    component along camera 0's gauge axis, which the gauge holds (at its true value here) and refine_poses adjusts: camera 1
    is compared without that component, and its other five parameters sit at the minimum of a problem with one constraint more.
    Measured once on the CPU references (HeldRefAdjuster with delta_tol 1e-14 against tests/_pose_ransac_ref.py::pose_refine with
    30 steps): cameras 2 .. 7 differ by at most 1.41e-10 (R and t; both iterations stop within that of their common
    minimum), camera 1 by 8.17e-4 in R and 7.89e-4 in t off the gauge axis (the constraint).  Asserted: ten times these."""
    sc = make_scene(300, 8, vis_p=0.5)
    m, g = 8, AXES[sc.axis]
    R0, t0 = sc.init_R.copy(), sc.init_t.copy()
    R0[0], t0[0] = sc.R_gt[0], sc.t_gt[0]
    axis0 = sc.R_gt[0][:, g]
    t0[1] += axis0 * (axis0 @ (sc.t_gt[1] - t0[1]))
    ba = BundleAdjuster.from_observations(sc.n_points, m, sc.pt_ptr, sc.cam_idx, sc.xy, sc.X_gt, sc.K_gt, R0, t0, axis=sc.axis,
                                          hold=["points", "intrinsics"])
    assert ba.n_held_points == sc.n_points and ba.n_free_camera_parameters == 6 * m - 7
    E0 = ba._engine.cost()
    X, K, R, t = ba.optimize(10.0, 1e-14, 50)
    assert np.array_equal(X, sc.X_gt) and np.array_equal(K, sc.K_gt) and ba._engine.cost() < 0.1 * E0
    Rr, tr, info = refine_poses(sc.X_gt, sc.pt_ptr, sc.cam_idx, sc.xy, sc.K_gt, R0, t0, n_steps=30)
    assert (info["status"] == 0).all()
    Rc, tc, _, _, st = PR.pose_refine(sc.X_gt, sc.pt_ptr, sc.cam_idx, sc.xy, sc.K_gt, R0, t0, n_steps=30)
    gap = max(np.abs(R[2:] - Rr[2:]).max(), np.abs(t[2:] - tr[2:]).max())
    d1 = t[1] - tr[1]
    gap1 = (np.abs(R[1] - Rr[1]).max(), np.abs(d1 - axis0 * (axis0 @ d1)).max())
    print(f"cameras 2..: {gap:.3e} (bound 1.41e-9); camera 1: R {gap1[0]:.3e} (8.17e-3), t off the gauge axis {gap1[1]:.3e} (7.89e-3); "
          f"refine_poses against its CPU reference: {max(np.abs(Rr - Rc).max(), np.abs(tr - tc).max()):.3e}")
    assert gap <= 10 * 1.41e-10
    assert gap1[0] <= 10 * 8.17e-4 and gap1[1] <= 10 * 7.89e-4
    assert np.abs(t[1:] - t0[1:]).max() > 1e-3  # (the poses did move)


# ---------------------------------------------------------------- 7: covariance
@pytest.mark.parametrize("name", ["one", "every_third", "all_but_one", "all", "random40"])
def test_covariance_with_held_points(golden, name):
    """DESIGN.md §11's bound, as tests/test_gpu_constraints.py::test_covariance_under_a_map: 1e-8 of the largest entry, against
    the dense reference (a); sigma2 as tests/test_gpu_constraints.py::test_adjuster_covariance_uses_the_free_count: 1e-9."""
    axis = "x-up_z-forward"
    d = golden("linearize_60x7_xup")
    n, m, pt_ptr, cam, xy, _, state = _golden_problem(d, axis)
    mask = masks(n)[name]
    kw = dict(hold="intrinsics") if name == "random40" else {}
    col, n_free = parameter_map(m, axis, **kw)
    eng = _mvba.HipEngine(n, m, pt_ptr, cam, xy, 1.0, axis)
    eng.set_params(*state)
    eng.set_parameter_map(col, n_free)
    eng.set_point_hold(mask)
    got = eng.covariance(full=True)
    for a, b in zip(eng.get_params(), state):
        assert np.array_equal(a, b)  # engine state bitwise untouched
    want = dense_covariance_held(n, m, pt_ptr, cam, xy, 1.0, col, n_free, mask, *state)
    for k in ("points", "cameras", "cameras_full"):
        if k == "points" and mask.all():
            continue  # (all zeros on both sides: asserted below)
        err = np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()
        print(name, k, f"max err / max entry = {err:.3e}")
        assert err <= 1e-8, k
    assert not got["points"][mask].any() and not want["points"][mask].any()
    assert mask.all() or (got["points"][~mask][:, [0, 1, 2], [0, 1, 2]] > 0).all()
    # the adjuster: zero blocks in either frame, sigma2 over 3 (N - n_held) + n_free unknowns
    ba = BundleAdjuster(d["x"], d["init_X"], d["init_K"], d["init_R"], d["init_t"], visibility_index=d["vis"] if "vis" in d.files else None,
                        axis=axis, hold_points=mask, **kw)
    res = ba.covariance(scale="residual", frame="input")
    E = ba._engine.cost()
    s2 = residual_variance(E, len(cam), n, m, n_free=n_free, n_held=int(mask.sum()))
    assert s2 == E / (2 * len(cam) - 3 * (n - int(mask.sum())) - n_free)
    assert res["sigma2"] == pytest.approx(s2, rel=1e-9)
    assert not res["points"][mask].any()


def test_covariance_stays_undefined_for_a_robust_engine():
    sc = make_scene(200, 6, vis_p=0.7)
    ba = BundleAdjuster.from_observations(sc.n_points, 6, sc.pt_ptr, sc.cam_idx, sc.xy, sc.init_X, sc.init_K, sc.init_R, sc.init_t,
                                          axis=sc.axis, hold_points=[0, 5], loss="cauchy", loss_scale=2.0)
    with pytest.raises(NotImplementedError):
        ba.covariance()


# ---------------------------------------------------------------- 8: the C ABI
def test_c_abi_state_and_arguments():
    n, m, pt_ptr, cam, xy, axis, state = _scene_problem(300, 4, 0.8)
    eng = _mvba.HipEngine(n, m, pt_ptr, cam, xy, 1.0, axis)
    eng.set_params(*state)
    lib, h = eng.lib, eng._h
    u8 = C.POINTER(C.c_uint8)
    held = np.zeros(n, np.uint8)
    held[[1, 7]] = (1, 200)  # nonzero = held
    assert lib.mvba_set_point_hold(None, held.ctypes.data_as(u8)) == _mvba.MVBA_ERR_BADARG
    eng.linearize()
    eng.try_step(1e-4)
    assert lib.mvba_set_point_hold(h, held.ctypes.data_as(u8)) == _mvba.MVBA_OK
    assert lib.mvba_commit(h) == _mvba.MVBA_ERR_STATE  # the trial is void,
    E = eng.try_step(1e-4)  # the linearisation is kept
    assert np.isfinite(E) and not eng.debug_read("dX").reshape(-1, 3)[[1, 7]].any()
    assert lib.mvba_triangulate_state(h, 2, None, None, None) == _mvba.MVBA_ERR_STATE
    assert b"clear the mask first" in lib.mvba_last_error()
    with pytest.raises(RuntimeError, match="2 points are held"):
        eng.triangulate()
    assert lib.mvba_commit(h) == _mvba.MVBA_OK  # (the refused call left the trial alone)
    with pytest.raises(ValueError, match=rf"shape \({n},\)"):
        eng.set_point_hold(np.zeros(n + 1, bool))
    with pytest.raises(ValueError, match="bool"):
        eng.set_point_hold(np.zeros(n, np.uint8))
    assert lib.mvba_set_point_hold(h, None) == _mvba.MVBA_OK
    _, status, _ = eng.triangulate()
    assert (status == 0).all()
