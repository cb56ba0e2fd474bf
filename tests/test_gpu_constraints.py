"""Parameter maps on the HIP engine (mvba_set_parameter_map) against the reference of
tests/_constraints_ref.py: one step for every kind of map, every route into the dense solve, whole trajectories, the
invariants (held = untouched, tied = equal, runs repeat bit for bit, the default map is the engine without maps), the
robust and the sharded engines, covariances, the C ABI's errors, and config 3 at full size.  Tolerances are those of the
existing test of the same quantity (tests/test_gpu_parity.py, tests/test_gpu_covariance.py); each is named at its assert."""
import numpy as np
import pytest

from _constraints_ref import (ConstrainedOracleEngine, ConstrainedRobustEngine, RefAdjuster, dense_covariance_mapped,
                              map_matrix)
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster, lm_loop, parameter_map, residual_variance, to_gauge_frame
from lib.synthetic import make_scene
from oracle import ba_oracle as O

pytestmark = pytest.mark.gpu


def _maps(m, axis):
    """The maps M of the issue: name -> (col, n_free)."""
    rng = np.random.default_rng(5)
    grp = np.zeros(m, int)
    grp[m // 3:] = 1  # two groups of unequal size
    return {
        "hold_intr": parameter_map(m, axis, hold="intrinsics"),
        "share_intr": parameter_map(m, axis, share="intrinsics"),
        "share_f_hold_u": parameter_map(m, axis, share="f", hold="u"),
        "two_groups": parameter_map(m, axis, share="intrinsics", share_groups=grp),
        "hold_pose": parameter_map(m, axis, hold="pose"),
        "random_mask": parameter_map(m, axis, hold=rng.random((m, 9)) < 0.4),
        "hold_all": parameter_map(m, axis, hold="cameras"),
    }


MAP_NAMES = ["hold_intr", "share_intr", "share_f_hold_u", "two_groups", "hold_pose", "random_mask", "hold_all"]


def _state(X, K, R, t, axis):
    Xg, Rg, tg = O.normalize_scene(X, R, t, axis)
    Km = np.array(K, float)
    Km[:] = Km.mean(axis=0)  # one camera body: tied parameters start equal
    return Xg, Km[:, 0, 0].copy(), Km[:, :2, 2].copy(), tg, Rg


def _pair(n, m, pt_ptr, cam, xy, axis, state, **kw):
    eng = _mvba.HipEngine(n, m, pt_ptr, cam, xy, 1.0, axis, **kw)
    ref = (ConstrainedRobustEngine if kw else ConstrainedOracleEngine)(n, m, pt_ptr, cam, np.asarray(xy).reshape(-1, 2), 1.0, axis, **kw)
    eng.set_params(*state)
    ref.set_params(*state)
    return eng, ref


def _golden_problem(d, axis):
    vis = d["vis"] if "vis" in d.files else None
    n, m = d["x"].shape[:2]
    pt_ptr, cam, xy = O.dense_to_observations(d["x"], vis)
    return n, m, pt_ptr, cam, xy, axis, _state(d["init_X"], d["init_K"], d["init_R"], d["init_t"], axis)


def _scene_problem(n, m, p):
    sc = make_scene(n, m, vis_p=p)
    return n, m, sc.pt_ptr, sc.cam_idx, sc.xy, sc.axis, _state(sc.init_X, sc.init_K, sc.init_R, sc.init_t, sc.axis)


def _check_step(eng, ref, col, n_free, c, dxi_tol=1e-9, e_tol=1e-12, dx_tol=1e-9, trial_tol=1e-10):
    """One trial of both engines (already linearised): dxi, dX, the trial state, the trial cost."""
    E, Eo = eng.try_step(c), ref.try_step(c)
    m = ref.m
    dxi_ref = map_matrix(col, n_free) @ ref.dxi_red if n_free else np.zeros(9 * m)
    dxi = eng.debug_read("dxi")
    print(f"n_free {n_free} c {c:g}: max|dxi - ref| / max|dxi| = {np.abs(dxi - dxi_ref).max() / max(np.abs(dxi_ref).max(), 1e-300):.3e}, "
          f"|E - Eo| / Eo = {abs(E - Eo) / Eo:.3e}")
    # tests/test_gpu_parity.py:56: 1e-9 of max|dxi|
    np.testing.assert_allclose(dxi, dxi_ref, rtol=0, atol=dxi_tol * np.abs(dxi_ref).max())
    assert (dxi[col < 0] == 0).all()
    for j in np.unique(col[col >= 0]):
        assert len(set(dxi[col == j].tolist())) == 1
    np.testing.assert_allclose(eng.debug_read("dX").reshape(-1, 3), ref.dX, rtol=0, atol=dx_tol * np.abs(ref.dX).max())
    np.testing.assert_allclose(eng.debug_read("trial_X").reshape(-1, 3), ref.tX, rtol=0, atol=trial_tol)
    tc = eng.debug_read("trial_cam").reshape(m, 15)
    np.testing.assert_allclose(tc[:, 0], ref.tf, atol=trial_tol)
    np.testing.assert_allclose(tc[:, 1:3], ref.tu, atol=trial_tol)
    np.testing.assert_allclose(tc[:, 3:6], ref.tt, atol=trial_tol)
    np.testing.assert_allclose(tc[:, 6:].reshape(-1, 3, 3), ref.tR, atol=trial_tol)
    assert E == pytest.approx(Eo, rel=e_tol)
    return E


# ---------------------------------------------------------------- 1: one step
@pytest.mark.parametrize("scene", ["linearize_60x7_xup", "linearize_60x7_xright", "2000x30"])
def test_one_step_for_every_kind_of_map(golden, scene):
    if scene == "2000x30":
        prob = _scene_problem(2000, 30, 0.3)
    else:
        prob = _golden_problem(golden(scene), "x-up_z-forward" if scene.endswith("xup") else "x-right_z-forward")
    n, m, pt_ptr, cam, xy, axis, state = prob
    eng, ref = _pair(*prob)
    eng.linearize()
    ref.linearize()
    base = {}
    for c in (1e-4, 1e-1):  # the default map's reduced system, from this very engine
        eng.try_step(c)
        base[c] = (eng.debug_read("A_full"), eng.debug_read("b_full"))
    for name, (col, n_free) in _maps(m, axis).items():
        eng.set_parameter_map(col, n_free)
        ref.set_parameter_map(col, n_free)
        assert eng.n_free == n_free
        for c in (1e-4, 1e-1):
            print(scene, name, end=" ")
            _check_step(eng, ref, col, n_free, c)
            assert np.array_equal(eng.debug_read("A_full"), base[c][0]) and np.array_equal(eng.debug_read("b_full"), base[c][1])
    assert eng.stats()["counts"]["lu_fallback"] == 0


# ---------------------------------------------------------------- 2: every route into the solve
ROUTES = [("pairs", (3000, 14, 0.5), {"MVBA_SCHUR": "pairs", "MVBA_FORCE_BIG": "1"}),
          ("slots", (3000, 14, 0.5), {"MVBA_SCHUR": "slots"}),
          ("lanes", (3000, 14, 0.5), {"MVBA_SCHUR": "lanes"}),  # one lane per item on the compact record (k_schur_lanes_compact)
          ("dense", (3001, 12, 1.0), {"MVBA_SCHUR": "dense"}),
          ("gcam647", (3000, 647, 0.04), {}),
          ("launches", (3000, 50, 0.3), {"MVBA_CHOL": "launches"}),
          ("polls0", (4000, 50, 0.2), {"MVBA_CHOL_BARRIER_POLLS": "0"}),
          ("check_solve", (3000, 300, 0.06), {"MVBA_CHECK_SOLVE": "1"})]


@pytest.mark.parametrize("route,shape,env", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("kind", ["hold_intr", "share_intr"])
def test_every_route_into_the_solve(route, shape, env, kind, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = _scene_problem(*shape)
    n, m, pt_ptr, cam, xy, axis, state = prob
    eng, ref = _pair(*prob)
    if route in ("pairs", "slots", "dense"):
        assert eng.schur_info()["kernel"] == route
    if route == "lanes":  # (reported as "slots"; step width 21 would be k_schur_slots, the fall-back)
        info = eng.schur_info()
        assert info["kernel"] == "slots" and info["step_width"] == 64 and info["record"] == "compact", info
        print(f"form {info['kernel']}, step width {info['step_width']}, record {info['record']}", end=" ")
    col, n_free = _maps(m, axis)[kind]
    eng.set_parameter_map(col, n_free)
    ref.set_parameter_map(col, n_free)
    eng.linearize()
    ref.linearize()
    print(route, kind, end=" ")
    if route == "gcam647":  # the bounds of test_extreme_camera_counts_vs_oracle: dxi 1e-7, cost 1e-7
        _check_step(eng, ref, col, n_free, 1e-2, dxi_tol=1e-7, e_tol=1e-7, dx_tol=1e-7, trial_tol=1e-7)
    else:
        _check_step(eng, ref, col, n_free, 1e-4)
    st = eng.stats()["counts"]
    assert st["lu_fallback"] == 0
    if route == "polls0":  # as test_barrier_timeout_...: a wait gives up at once where the grid has waits (more than one super-block)
        assert st["barrier_fallback"] == (1 if n_free > 128 else 0)


@pytest.mark.parametrize("shape", [(400, 6, 0.7), (2500, 75, 0.2)])
@pytest.mark.parametrize("kind", ["hold_intr", "share_intr"])
def test_indefinite_mapped_system_takes_the_lu_rescue(shape, kind):
    """As test_indefinite_reduced_system_takes_the_lu_path_like_numpy, same bounds (dxi 1e-8, cost 1e-6)."""
    prob = _scene_problem(*shape)
    n, m, pt_ptr, cam, xy, axis, state = prob
    eng, ref = _pair(*prob)
    col, n_free = _maps(m, axis)[kind]
    eng.set_parameter_map(col, n_free)
    ref.set_parameter_map(col, n_free)
    eng.linearize()
    ref.linearize()
    _check_step(eng, ref, col, n_free, -1.5, dxi_tol=1e-8, e_tol=1e-6, dx_tol=1e-6, trial_tol=1e-6)
    w = np.linalg.eigvalsh(ref.A)
    assert w.min() < 0 < w.max()
    assert eng.stats()["counts"]["lu_fallback"] == 1
    _check_step(eng, ref, col, n_free, 1e-4)
    assert eng.stats()["counts"]["lu_fallback"] == 1


def test_check_solve_fires_on_a_mapped_system(monkeypatch):
    monkeypatch.setenv("MVBA_CHECK_SOLVE", "1e-30")  # an impossible tolerance, as the existing test of the check
    prob = _scene_problem(3000, 30, 0.3)
    eng, _ = _pair(*prob)
    eng.set_parameter_map(*_maps(30, prob[5])["share_intr"])
    eng.linearize()
    with pytest.raises(RuntimeError, match="MVBA_CHECK_SOLVE"):
        eng.try_step(1e-4)


# ---------------------------------------------------------------- 3: trajectories
TRAJ = [("linearize_60x7_xup", "x-up_z-forward", (10.0, 1e-8, 8)), ("linearize_60x7_xright", "x-right_z-forward", (10.0, 1e-8, 8)),
        ("visibility_300x12", "x-up_z-forward", (2.0, 1e-10, 10))]
# (visibility_300x12 stops on delta_tol = 1e-10, not after 10 iterations with delta_tol = -1 as the default-map test runs it: the
# mapped problems converge in about seven iterations, and the iterations after that sit on the rounding floor (|dE| ~ 1e-18),
# where the strict accept test E' > E is a coin toss -- the reference took 47 solves there, the engine 11.
# tests/test_constraints_cpu.py checks that the reference keeps its counts on these cases when A is perturbed by 1e-13.)
TRAJ_MAPS = {"hold_intr": dict(hold="intrinsics"), "share_intr": dict(share="intrinsics"), "share_f_hold_u": dict(share="f", hold="u")}


@pytest.mark.parametrize("name,axis,args", TRAJ, ids=[t[0] for t in TRAJ])
@pytest.mark.parametrize("kind", list(TRAJ_MAPS))
def test_trajectory_vs_reference(golden, name, axis, args, kind):
    """The bounds of test_full_trajectory_vs_reference: equal counts, every logged cost 1e-9 relative, outputs 1e-9."""
    d = golden(name)
    vis = d["vis"] if "vis" in d.files else None
    K = d["init_K"].copy()
    K[:] = K.mean(axis=0)
    out = []
    for cls in (BundleAdjuster, RefAdjuster):
        ba = cls(d["x"], d["init_X"], K, d["init_R"], d["init_t"], visibility_index=vis, axis=axis, **TRAJ_MAPS[kind])
        res = ba.optimize(*args, is_debug=True)
        out.append((res, np.array([e["reprojection_error"] for e in ba.get_log()]), ba._engine.n_solves))
    (got, E, ns), (want, Eo, nso) = out
    print(name, kind, "outer", len(E) - 1, len(Eo) - 1, "solves", ns, nso, "max rel dE", np.abs(E[:len(Eo)] / Eo[:len(E)] - 1).max())
    assert len(E) == len(Eo) and ns == nso
    np.testing.assert_allclose(E, Eo, rtol=1e-9, atol=1e-12)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)


# ---------------------------------------------------------------- 4: invariants
def _adjust(sc, K, **kw):
    ba = BundleAdjuster.from_observations(sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, sc.init_X, K, sc.init_R,
                                          sc.init_t, axis=sc.axis, **kw)
    return ba


def test_held_stay_tied_stay_equal_and_runs_repeat_bitwise():
    sc = make_scene(2000, 30, vis_p=0.3)
    K = sc.init_K.copy()
    K[:] = K.mean(axis=0)
    grp = np.arange(30) % 3
    mask = np.random.default_rng(2).random((30, 9)) < 0.3
    for kw in (dict(hold="intrinsics"), dict(share="intrinsics"), dict(share="f", hold="u"),
               dict(share="intrinsics", share_groups=grp), dict(hold="pose"), dict(hold=mask), dict(hold="cameras")):
        col, n_free = parameter_map(30, sc.axis, **kw)
        runs = []
        for _ in range(2):
            ba = _adjust(sc, K, **kw)
            eng = ba._engine
            before = eng.get_params()
            E0 = eng.cost()
            E = lm_loop(eng, 10.0, 1e-10, 6, verbose=False)  # in the gauge frame, where "held" is meant
            runs.append((E,) + tuple(eng.get_params()))
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a, b)
        assert runs[0][0] < E0
        _, X, f, u, t, R = runs[0]
        cam_before = np.concatenate([before[1][:, None], before[2], before[3]], axis=1)  # (m, 6): f, u, v, t
        cam_after = np.concatenate([f[:, None], u, t], axis=1)
        col9 = col.reshape(30, 9)
        assert np.array_equal(cam_after[col9[:, :6] < 0], cam_before[col9[:, :6] < 0])
        fixed_R = (col9[:, 6:] < 0).all(axis=1)
        assert np.array_equal(R[fixed_R], before[4][fixed_R])
        if n_free:
            assert not np.array_equal(cam_after[col9[:, :6] >= 0], cam_before[col9[:, :6] >= 0])
        for j in np.unique(col[col >= 0]):
            g = np.nonzero(col == j)[0]
            if len(g) > 1:  # (tied slots are intrinsics)
                assert len(set(cam_after[g // 9, g % 9].tolist())) == 1


def test_default_map_is_the_engine_that_never_heard_of_maps():
    sc = make_scene(2000, 30, vis_p=0.3)
    prob = (sc.n_points, 30, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis)
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    state = (X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    out = []
    for how in ("never", "explicit", "map_then_null"):
        eng = _mvba.HipEngine(*prob)
        eng.set_params(*state)
        if how == "explicit":
            eng.set_parameter_map(*parameter_map(30, sc.axis))
        if how == "map_then_null":
            eng.set_parameter_map(*parameter_map(30, sc.axis, hold="intrinsics"))
            eng.linearize()
            eng.try_step(1e-4)
            eng.set_parameter_map(None)
        assert eng.n_free == 9 * 30 - 7
        Es = [eng.cost()]
        eng.n_solves = 0  # (the binding's counter: the trial under the other map is not part of the run compared here)
        lm_loop(eng, 10.0, -1.0, 5, on_state=Es.append, verbose=False)
        out.append((np.array(Es), eng.n_solves) + tuple(eng.get_params()))
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(a, b)


def test_everything_held_runs_and_matches_the_reference():
    prob = _scene_problem(2000, 30, 0.3)
    eng, ref = _pair(*prob)
    col, n_free = parameter_map(30, prob[5], hold="cameras")
    assert n_free == 0
    eng.set_parameter_map(col, n_free)
    ref.set_parameter_map(col, n_free)
    Es, Eo = [eng.cost()], [ref.cost()]
    lm_loop(eng, 10.0, 1e-10, 8, on_state=Es.append, verbose=False)
    lm_loop(ref, 10.0, 1e-10, 8, on_state=Eo.append, verbose=False)
    assert len(Es) == len(Eo) and eng.n_solves == ref.n_solves
    np.testing.assert_allclose(Es, Eo, rtol=1e-9)
    for a, b in zip(eng.get_params()[1:], prob[6][1:]):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(eng.get_params()[0], ref.get_params()[0], rtol=0, atol=1e-9)


# ---------------------------------------------------------------- 5: with the neighbours
def test_huber_with_held_intrinsics():
    from _robust_ref import inject_outliers

    sc = make_scene(2000, 16, vis_p=0.4)
    xy, _ = inject_outliers(sc.xy, 0.05, 20.0, 100.0, seed=3)
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    state = (X, sc.init_K[:, 0, 0].copy(), sc.init_K[:, :2, 2].copy(), t, R)  # calibrated cameras: each its own known intrinsics
    eng, ref = _pair(sc.n_points, 16, sc.pt_ptr, sc.cam_idx, xy, sc.axis, state, loss="huber", loss_scale=2.0)
    col, n_free = parameter_map(16, sc.axis, hold="intrinsics")
    eng.set_parameter_map(col, n_free)
    ref.set_parameter_map(col, n_free)
    assert eng.cost() == pytest.approx(ref.cost(), rel=1e-12)
    eng.linearize()
    ref.linearize()
    _check_step(eng, ref, col, n_free, 1e-4, e_tol=1e-9)  # (the robust trial cost: the bound of tests/test_gpu_robust.py:60)
    assert np.array_equal(eng.debug_read("dxi").reshape(16, 9)[:, :3], np.zeros((16, 3)))


def test_huber_trajectory_with_held_intrinsics(golden):
    """tests/test_gpu_robust.py::test_trajectory_matches_the_reference_lm_loop (its scene, its outliers, its bounds) with
    hold="intrinsics" on both sides.  (Measured on the one-step scene above instead: lm_loop for four iterations after that
    step gave costs 1.3e-7 apart although every single trial, compared at the same state and damping, agreed to 4e-12 --
    DESIGN.md §13; this scene's reference keeps its costs to 2e-14 when A is perturbed by 1e-13.)"""
    name, axis, args = "linearize_60x7_xright", "x-right_z-forward", (10.0, 1e-8, 8)
    d = golden(name)
    x = np.array(d["x"], np.float64, copy=True)
    live = np.argwhere(np.ones(x.shape[:2], bool))
    rng = np.random.default_rng(11)
    pick = live[rng.choice(len(live), size=max(1, len(live) // 15), replace=False)]
    ang = rng.uniform(0, 2 * np.pi, len(pick))
    r = rng.uniform(20.0, 100.0, len(pick))
    x[pick[:, 0], pick[:, 1]] += np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    ba = BundleAdjuster(x, d["init_X"], d["init_K"], d["init_R"], d["init_t"], axis=axis, loss="huber", loss_scale=2.0, hold="intrinsics")
    X, K, R, t = ba.optimize(*args, is_debug=True)
    E = np.array([e["reprojection_error"] for e in ba.get_log()])
    n, m = x.shape[:2]
    pt_ptr, cam, xy = O.dense_to_observations(x, None)
    g = ConstrainedRobustEngine(n, m, pt_ptr, cam, xy, 1.0, axis, loss="huber", loss_scale=2.0)
    Xg, Rg, tg = O.normalize_scene(d["init_X"], d["init_R"], d["init_t"], axis)
    g.set_params(Xg, d["init_K"][:, 0, 0], d["init_K"][:, :2, 2], tg, Rg)
    g.set_parameter_map(*parameter_map(m, axis, hold="intrinsics"))
    Es = []
    lm_loop(g, *args, on_state=Es.append, verbose=False)
    print("huber trajectory: outer", len(E) - 1, len(Es) - 1, "solves", ba._engine.n_solves, g.n_solves)
    assert len(E) == len(Es) and ba._engine.n_solves == g.n_solves
    np.testing.assert_allclose(E, Es, rtol=1e-9, atol=1e-12)
    assert np.array_equal(K[:, 0, 0], d["init_K"][:, 0, 0]) and np.array_equal(K[:, :2, 2], d["init_K"][:, :2, 2])
    log = ba.get_log()
    np.testing.assert_allclose(log[-1]["points"], g.get_params()[0], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(log[-1]["pos"], g.get_params()[3], rtol=1e-9, atol=1e-9)


def test_two_thread_ranks_host_transport_with_shared_intrinsics():
    from lib import _distributed as D

    n, m, pt_ptr, cam, xy, axis, state = _scene_problem(3000, 20, 0.3)
    X, f, u, t, R = state
    col, n_free = parameter_map(m, axis, share="intrinsics")
    one = _mvba.HipEngine(n, m, pt_ptr, cam, xy, 1.0, axis)
    one.set_params(*state)
    one.set_parameter_map(col, n_free)
    E_one = [one.cost()]
    lm_loop(one, 2.0, -1.0, 4, on_state=E_one.append, verbose=False)
    parts = D.partition_points(pt_ptr, 2)

    def body(rank, g):
        lo, hi = parts[rank]
        p2, c2, x2 = D.slice_observations(pt_ptr, cam, xy, lo, hi)
        eng = _mvba.HipEngine(hi - lo, m, p2, c2, x2, 1.0, axis)
        g.attach(eng, rank)
        eng.set_params(X[lo:hi], f, u, t, R)
        eng.set_parameter_map(col, n_free)  # the same map on every rank
        Es = [eng.cost()]
        lm_loop(eng, 2.0, -1.0, 4, on_state=Es.append, verbose=False)
        return Es, eng.get_params()

    res = D.InProcessGroup(2).run(body)
    for r in res:
        np.testing.assert_allclose(r[0], E_one, rtol=1e-14)
    for i in (1, 2, 3, 4):
        assert np.array_equal(res[0][1][i], res[1][1][i])
    assert len(set(res[0][1][1].tolist())) == 1  # one focal length
    np.testing.assert_allclose(res[0][1][1], one.get_params()[1], rtol=1e-9)


# ---------------------------------------------------------------- 6: covariance
@pytest.mark.parametrize("scene", ["linearize_60x7_xup", "linearize_60x7_xright", "200x6"])
@pytest.mark.parametrize("kind", ["hold_intr", "share_intr"])
def test_covariance_under_a_map(golden, scene, kind):
    """DESIGN.md §11's bound: 1e-8 of the largest entry, against the dense reference."""
    if scene == "200x6":
        prob = _scene_problem(200, 6, 0.7)
    else:
        prob = _golden_problem(golden(scene), "x-up_z-forward" if scene.endswith("xup") else "x-right_z-forward")
    n, m, pt_ptr, cam, xy, axis, state = prob
    eng = _mvba.HipEngine(n, m, pt_ptr, cam, xy, 1.0, axis)
    eng.set_params(*state)
    col, n_free = _maps(m, axis)[kind]
    eng.set_parameter_map(col, n_free)
    got = eng.covariance(full=True)
    after = eng.get_params()
    for a, b in zip(after, state):
        assert np.array_equal(a, b)  # engine state bitwise untouched
    want = dense_covariance_mapped(n, m, pt_ptr, cam, xy, 1.0, col, n_free, *state)
    for k in ("points", "cameras", "cameras_full"):
        err = np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()
        print(scene, kind, k, f"max err / max entry = {err:.3e}")
        assert err <= 1e-8, k
    Cf = got["cameras_full"]
    held = np.nonzero(col < 0)[0]
    assert (Cf[held] == 0).all() and (Cf[:, held] == 0).all()
    for j in np.unique(col[col >= 0]):
        g = np.nonzero(col == j)[0]
        for q in g[1:]:
            assert np.array_equal(Cf[q], Cf[g[0]]) and np.array_equal(Cf[:, q], Cf[:, g[0]])
    # cameras_full = P Sigma' P^T: every entry is the entry of its pair of unknowns
    free = np.nonzero(col >= 0)[0]
    first = np.array([np.nonzero(col == j)[0][0] for j in range(n_free)])
    Sig = Cf[np.ix_(first, first)]
    assert np.array_equal(Cf[np.ix_(free, free)], Sig[np.ix_(col[free], col[free])])
    assert np.array_equal(Cf, Cf.T)


def test_adjuster_covariance_uses_the_free_count():
    sc = make_scene(200, 6, vis_p=0.7)
    K = sc.init_K.copy()
    K[:] = K.mean(axis=0)
    ba = _adjust(sc, K, share="intrinsics")
    ba.optimize(10.0, 1e-10, 20)
    unit = ba.covariance(scale="unit", frame="gauge")
    res = ba.covariance(scale="residual", frame="gauge")
    n_free = ba.n_free_camera_parameters
    assert n_free == 9 * 6 - 7 - 18 + 3
    X, f, u, t, R = ba._engine.get_params()
    Xg, Rg, tg = to_gauge_frame(X, R, t, sc.axis)
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    E = O.cost(Xg, f, u, tg, Rg, 1.0, pt, sc.cam_idx, sc.xy)
    s2 = residual_variance(E, sc.n_obs, sc.n_points, 6, n_free=n_free)
    assert s2 == E / (2 * sc.n_obs - 3 * sc.n_points - n_free)
    assert res["sigma2"] == pytest.approx(s2, rel=1e-9)
    np.testing.assert_allclose(res["cameras"], unit["cameras"] * res["sigma2"], rtol=1e-12)
    inp = ba.covariance(scale="unit", frame="input")  # T acts on t and omega only: intrinsics as in the gauge frame
    np.testing.assert_allclose(inp["cameras"][:, :3, :3], unit["cameras"][:, :3, :3], rtol=1e-12)


# ---------------------------------------------------------------- 7: errors
def test_c_abi_rules_and_state():
    n, m, pt_ptr, cam, xy, axis, state = _scene_problem(300, 4, 0.8)
    eng = _mvba.HipEngine(n, m, pt_ptr, cam, xy, 1.0, axis)
    eng.set_params(*state)
    good, n_free = parameter_map(m, axis, share="f")

    def bad(change, n=None):
        col = good.copy()
        change(col)
        return col, n_free if n is None else n

    def set_(col, i, v):
        col[i] = v

    gauge = 12 + (1 if axis == "x-up_z-forward" else 0)
    cases = [(bad(lambda c: set_(c, 4, 0)), r"col\[4\] is a gauge slot"),
             (bad(lambda c: set_(c, gauge, 1)), rf"col\[{gauge}\] is a gauge slot"),
             (bad(lambda c: set_(c, 10, n_free)), r"col\[10\] = \d+ is neither -1 nor below n_free"),
             (bad(lambda c: set_(c, 10, -2)), r"col\[10\] = -2"),
             (bad(lambda c: None, n_free + 1), rf"unknown {n_free} has no parameter slot"),
             (bad(lambda c: set_(c, 11, good[1])), r"col\[11\] ties slot 11 to slot 1"),  # v tied to u: different p
             (bad(lambda c: set_(c, 24, good[15])), r"col\[24\] ties slot 24 to slot 15"),  # omega_x of two cameras: p > 2
             ((good, 9 * m), r"n_free = \d+ must be in 0")]
    for (col, nf), msg in cases:
        with pytest.raises(ValueError, match=msg):
            eng.set_parameter_map(col, nf)
    with pytest.raises(ValueError, match="9 n_images"):
        eng.set_parameter_map(good[:-1], n_free)
    # a rejected map leaves the engine as it was; an accepted one voids the trial and keeps the linearisation
    eng.linearize()
    eng.try_step(1e-4)
    eng.set_parameter_map(good, n_free)
    with pytest.raises(RuntimeError, match="commit without a trial step"):
        eng.commit()
    E = eng.try_step(1e-4)  # no new linearize needed
    assert np.isfinite(E)
    eng.commit()


# ---------------------------------------------------------------- 8: full size
@pytest.mark.parametrize("kind", ["share_intr", "hold_intr"])
def test_config3_full_size(kind, monkeypatch):
    """BASELINE config 3 (1 M points x 100 cameras x 10 %), five LM iterations: the cost strictly falls, held parameters are
    bitwise untouched, tied ones bitwise equal, MVBA_CHECK_SOLVE passes on the first solve."""
    m = 100
    sc = make_scene(1_000_000, m, vis_p=0.1)
    state = _state(sc.init_X, sc.init_K, sc.init_R, sc.init_t, sc.axis)
    col, n_free = _maps(m, sc.axis)[kind]
    monkeypatch.setenv("MVBA_CHECK_SOLVE", "1")
    chk = _mvba.HipEngine(sc.n_points, m, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis)
    monkeypatch.delenv("MVBA_CHECK_SOLVE")
    chk.set_params(*state)
    chk.set_parameter_map(col, n_free)
    chk.linearize()
    E1 = chk.try_step(1e-4)  # (raises if the check fails)
    chk.close()
    eng = _mvba.HipEngine(sc.n_points, m, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis)
    eng.set_params(*state)
    eng.set_parameter_map(col, n_free)
    Es = []  # (lm_loop reports the starting cost itself)
    lm_loop(eng, 10.0, -1.0, 5, on_state=Es.append, verbose=False)
    print(kind, "costs", Es)
    assert Es[1] == E1
    assert all(b < a for a, b in zip(Es, Es[1:]))
    X, f, u, t, R = eng.get_params()
    if kind == "hold_intr":
        assert np.array_equal(f, state[1]) and np.array_equal(u, state[2])
    else:
        assert len(set(f.tolist())) == 1 and len(set(u[:, 0].tolist())) == 1 and len(set(u[:, 1].tolist())) == 1
        assert f[0] != state[1][0]
    assert np.array_equal(t[0], state[3][0]) and np.array_equal(R[0], state[4][0])
    assert eng.stats()["counts"]["lu_fallback"] == 0
