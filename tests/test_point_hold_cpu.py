"""Held points without a GPU: the two references of tests/_point_hold_ref.py against each other, the Python front end
(hold_points / hold="points") and its errors, the count of unknowns in residual_variance, and the product's BundleAdjuster
over reference (b)."""
import numpy as np
import pytest

from _constraints_ref import ConstrainedOracleEngine, map_matrix
from _point_hold_ref import HeldOracleEngine, HeldRefAdjuster, dense_covariance_held, dense_step, masks
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster, parameter_map, point_hold_mask, residual_variance
from lib.synthetic import make_scene
from oracle import ba_oracle as O

AXIS = "x-up_z-forward"


def _golden_problem(d):
    n, m = d["x"].shape[:2]
    pt_ptr, cam, xy = O.dense_to_observations(d["x"], d["vis"] if "vis" in d.files else None)
    Xg, Rg, tg = O.normalize_scene(d["init_X"], d["init_R"], d["init_t"], AXIS)
    K = np.array(d["init_K"], float)
    K[:] = K.mean(axis=0)
    return n, m, pt_ptr, cam, xy, (Xg, K[:, 0, 0].copy(), K[:, :2, 2].copy(), tg, Rg)


def _close(a, b, tol, what):
    scale = max(np.abs(b).max(), 1e-300)
    err = np.abs(a - b).max()
    print(f"{what}: max err / max entry = {err / scale:.3e}")
    assert err <= tol * scale, (what, err, scale)


# ---------------------------------------------------------------- the two references
@pytest.mark.parametrize("name", ["one", "every_third", "all_but_one", "all", "random40"])
def test_dense_and_engine_references_agree(golden, name):
    """(a) deletes the held points' columns from J and solves the damped normal equations in one piece; (b) zeroes E_a^-1
    and goes through the Schur complement.  Bound: 2e-9 of the largest entry, the one at which tests/test_covariance_cpu.py
    holds the Schur-based reference to the dense one on this 60 x 7 scene (its golden_60x7 case) -- the two constructions
    here are that pair with columns deleted.  (tests/test_constraints_cpu.py itself compares its engine to the oracle bit for
    bit, under the default map; that comparison, for the empty mask, is the last test of this file.)  Measured: 2e-12."""
    n, m, pt_ptr, cam, xy, state = _golden_problem(golden("linearize_60x7_xup"))
    mask = masks(n)[name]
    col, n_free = parameter_map(m, AXIS, hold="intrinsics") if name == "random40" else parameter_map(m, AXIS)
    g = HeldOracleEngine(n, m, pt_ptr, cam, xy, 1.0, AXIS)
    g.set_params(*state)
    g.set_parameter_map(col, n_free)
    g.set_point_hold(mask)
    assert g.n_held_points == mask.sum()
    g.linearize()
    for c in (1e-4, 1e-1):
        g.try_step(c)
        a = dense_step(n, m, pt_ptr, cam, xy, 1.0, col, n_free, mask, c, *state)
        _close(map_matrix(col, n_free) @ g.dxi_red, a["dxi"], 2e-9, f"{name} c={c:g} dxi")
        if not mask.all():
            _close(g.dX, a["dX"], 2e-9, f"{name} c={c:g} dX")
        assert (g.dX[mask] == 0).all() and np.array_equal(g.tX[mask], state[0][mask])
        assert mask.all() or (g.dX[~mask] != 0).any()
    # the covariance of (a) against the one built from (b)'s undamped reduced system: Sigma = S^-1 over the free unknowns,
    # C_cam = 2 P Sigma P^T, C_a = 2 (E^-1 + E^-1 F Sigma F^T E^-1) at free points
    A, _ = g.reduced_system(0.0)
    P = map_matrix(col, n_free)
    Sig = P @ np.linalg.inv(P.T @ A @ P) @ P.T
    want = dense_covariance_held(n, m, pt_ptr, cam, xy, 1.0, col, n_free, mask, *state)
    _close(2.0 * Sig, want["cameras_full"], 2e-9, f"{name} cameras_full")
    Y = np.einsum("oij,ojk->oik", g.Einv[g.pt], g.F)  # E^-1 F per observation (zero rows at held points)
    pts = 2.0 * g.Einv.copy()
    for a_ in range(n):
        o = np.arange(pt_ptr[a_], pt_ptr[a_ + 1])
        W = np.concatenate([Y[i] for i in o], axis=1)  # 3 x 9 deg
        idx = np.concatenate([9 * cam[i] + np.arange(9) for i in o])
        pts[a_] += 2.0 * W @ Sig[np.ix_(idx, idx)] @ W.T
    _close(pts, want["points"], 2e-9, f"{name} points")
    assert not want["points"][mask].any() and not pts[mask].any()


def test_empty_mask_is_the_oracle_itself():
    sc = make_scene(60, 5, 0.8, project="numpy")
    args = (sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis)
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    engines = [HeldOracleEngine(*args), HeldOracleEngine(*args), HeldOracleEngine(*args), ConstrainedOracleEngine(*args)]
    engines[0].set_point_hold(np.zeros(sc.n_points, bool))
    engines[1].set_point_hold(np.arange(sc.n_points) % 2 == 0)
    engines[1].set_point_hold(None)
    for e in engines:
        e.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    o = engines[-1]
    for c in (1e-4, 1e-1):
        for e in engines:
            e.linearize()
        Eo = o.try_step(c)
        for g in engines[:-1]:
            assert g.try_step(c) == Eo and g.n_held_points == 0
            assert np.array_equal(g.dxi_red, o.dxi_red) and np.array_equal(g.dX, o.dX) and np.array_equal(g.A, o.A)
        for e in engines:
            e.commit()
    for g in engines[:-1]:
        for a, b in zip(g.get_params(), o.get_params()):
            assert np.array_equal(a, b)


def test_a_held_point_seen_once_is_legal_a_free_one_is_not():
    sc = make_scene(40, 4, 1.0, project="numpy")
    keep = np.ones(len(sc.cam_idx), bool)
    for a in (3, 17):  # these two keep their first observation only
        keep[sc.pt_ptr[a] + 1:sc.pt_ptr[a + 1]] = False
    deg = np.add.reduceat(keep.astype(np.int64), sc.pt_ptr[:-1])
    pt_ptr = np.concatenate([[0], np.cumsum(deg)])
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    g = HeldOracleEngine(sc.n_points, sc.n_images, pt_ptr, sc.cam_idx[keep], sc.xy[keep], 1.0, sc.axis)
    g.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    g.linearize()
    mask = np.zeros(sc.n_points, bool)
    mask[[3, 17]] = True
    # E_a of a point seen once has rank 2: undamped (the covariance's c = 0), np.linalg.inv either raises or returns an
    # inverse of rounding noise (which of the two depends on the last bit of an elimination)
    assert (np.linalg.cond(g.E[mask]) > 1e12).all() and (np.linalg.cond(g.E[~mask]) < 1e12).all()
    try:
        g.reduced_system(0.0)
        assert np.abs(g.Einv[mask]).max() > 1e10 * np.abs(g.Einv[~mask]).max()
    except np.linalg.LinAlgError:
        pass
    g.set_point_hold(mask)
    for c in (0.0, 1e-4):
        assert np.isfinite(g.try_step(c)) and (g.dX[mask] == 0).all() and not g.Einv[mask].any()
        assert np.abs(g.dX).max() < 1.0  # (an ordinary step)


# ---------------------------------------------------------------- the front end
def test_point_hold_mask_forms_and_errors():
    assert point_hold_mask(5, [1, 3]).tolist() == [False, True, False, True, False]
    assert point_hold_mask(5, np.array([4, 4, 0], np.int32)).tolist() == [True, False, False, False, True]
    assert point_hold_mask(3, np.array([True, False, True])).tolist() == [True, False, True]
    assert point_hold_mask(3, np.zeros(0, np.int64)).tolist() == [False] * 3
    with pytest.raises(ValueError, match=r"must have shape \(5,\), got \(4,\)"):
        point_hold_mask(5, np.zeros(4, bool))
    with pytest.raises(ValueError, match="float64"):
        point_hold_mask(5, np.array([1.0, 2.0]))
    with pytest.raises(ValueError, match=r"int64 \(2, 2\)"):
        point_hold_mask(5, np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError, match=r"index 5 \(entry 1\) is outside 0 \.\. 4"):
        point_hold_mask(5, [0, 5])
    with pytest.raises(ValueError, match="index -1"):
        point_hold_mask(5, [-1])
    X = np.zeros((5, 3))
    X[2, 1] = np.nan
    assert point_hold_mask(5, [1, 3], X).sum() == 2  # (a free point may start anywhere)
    with pytest.raises(ValueError, match="held point 2 starts from a position that is not finite"):
        point_hold_mask(5, [1, 2], X)


def test_adjuster_errors_come_before_any_device_work(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_mvba, "load_library", no_library)
    monkeypatch.setattr(_mvba, "device_count", no_library)
    sc = make_scene(20, 3, vis_p=1.0, project="numpy")
    head = (sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy)
    tail = (sc.init_K, sc.init_R, sc.init_t)
    Xnan = sc.init_X.copy()
    Xnan[7] = np.inf
    cases = [(sc.init_X, dict(hold_points=np.zeros(19, bool)), r"shape \(20,\), got \(19,\)"),
             (sc.init_X, dict(hold_points=np.array([0.5])), "float64"),
             (sc.init_X, dict(hold_points=[3, 20]), r"index 20 \(entry 1\) is outside 0 \.\. 19"),
             (None, dict(hold_points=[3]), r"hold_points with init_X=None: the 20 points"),
             (None, dict(hold="points"), r"hold_points with init_X=None: the 20 points"),
             (Xnan, dict(hold_points=[1, 7]), "held point 7 starts from a position that is not finite"),
             (Xnan, dict(hold=["points", "intrinsics"]), "held point 7"),
             (sc.init_X, dict(hold=["points", "focal"]), "unknown name 'focal'")]
    for X, kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            BundleAdjuster.from_observations(*head, X, *tail, axis=sc.axis, **kw)
    x = np.zeros((sc.n_points, sc.n_images, 2))
    with pytest.raises(ValueError, match="index 20"):
        BundleAdjuster(x, sc.init_X, *tail, axis=sc.axis, hold_points=[20])
    with pytest.raises(ValueError, match="init_X=None"):
        BundleAdjuster(x, None, *tail, axis=sc.axis, hold_points=[2])


def test_binding_and_header_declare_the_entry_point():
    hdr = open(_mvba.os.path.join(_mvba.os.path.dirname(_mvba._HERE), "..", "include", "mvba.h")).read()
    assert "int mvba_set_point_hold(mvba_handle *h, const uint8_t *held);" in hdr
    assert "mvba_set_point_hold" in _mvba.SIGNATURES


def test_residual_variance_counts_held_points_out():
    assert residual_variance(3.0, 100, 10, 4, n_held=0) == residual_variance(3.0, 100, 10, 4) == 3.0 / (200 - 59)
    assert residual_variance(3.0, 100, 10, 4, n_held=4) == 3.0 / (200 - (18 + 29))
    assert residual_variance(3.0, 100, 10, 4, n_free=17, n_held=10) == 3.0 / (200 - 17)
    assert residual_variance(3.0, 100, 10, 4, 17, 3) == 3.0 / (200 - (21 + 17))
    with pytest.raises(ValueError, match="no redundancy"):
        residual_variance(1.0, 20, 10, 2)
    assert residual_variance(1.0, 20, 10, 2, n_held=5) == 1.0 / (40 - 15 - 11)  # holding points restores the redundancy


# ---------------------------------------------------------------- BundleAdjuster over reference (b)
@pytest.fixture(scope="module")
def runs():
    sc = make_scene(300, 8, 0.7, project="numpy")
    args = (sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, sc.init_X, sc.init_K, sc.init_R, sc.init_t)
    half = np.arange(sc.n_points) % 2 == 0
    out = {}
    for name, kw in (("free", {}), ("half", dict(hold_points=half)), ("half_idx", dict(hold_points=np.nonzero(half)[0])),
                     ("all", dict(hold="points")), ("all_intr", dict(hold=["points", "intrinsics"])),
                     ("huber_half", dict(hold_points=half, loss="huber", loss_scale=2.0))):
        ba = HeldRefAdjuster.from_observations(*args, axis=sc.axis, **kw)
        E0 = ba._engine.cost()
        X, K, R, t = ba.optimize(10.0, 1e-10, 30)
        out[name] = dict(ba=ba, E0=E0, E=ba._engine.cost(), X=X, K=K, R=R, t=t)
    return sc, half, out


def test_held_points_come_back_bit_for_bit(runs):
    sc, half, out = runs
    for name in ("half", "half_idx", "huber_half"):
        assert np.array_equal(out[name]["X"][half], sc.init_X[half]) and out[name]["ba"].n_held_points == half.sum()
        assert not np.array_equal(out[name]["X"][~half], sc.init_X[~half])
    for a, b in zip((out["half"][k] for k in "XKRt"), (out["half_idx"][k] for k in "XKRt")):
        assert np.array_equal(a, b)  # a mask and the indices of its True entries are one thing
    for name in ("all", "all_intr"):
        assert np.array_equal(out[name]["X"], sc.init_X) and out[name]["ba"].n_held_points == sc.n_points
        assert not np.array_equal(out[name]["t"], sc.init_t)
    assert np.array_equal(out["all_intr"]["K"], sc.init_K) and not np.array_equal(out["all"]["K"], sc.init_K)
    assert out["all_intr"]["ba"].n_free_camera_parameters == 9 * 8 - 7 - 24 and out["free"]["ba"].n_held_points == 0


def test_costs_fall_and_nest(runs):
    """Holding points is a sub-model: E_all_intr >= E_all >= E_half >= E_free at convergence."""
    _, _, out = runs
    for name, r in out.items():
        assert r["E"] < r["E0"], name
    E = {k: v["E"] for k, v in out.items()}
    assert E["all_intr"] >= E["all"] - 1e-12 and E["all"] >= E["half"] - 1e-12 and E["half"] >= E["free"] - 1e-12
