"""Parameter maps without a GPU: the map front end (lib.bundle_adjustment.parameter_map), the reference engine of
tests/_constraints_ref.py, and the product's BundleAdjuster over that reference (hold / share / share_groups)."""
import numpy as np
import pytest

from _constraints_ref import ConstrainedOracleEngine, RefAdjuster, map_matrix
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster, parameter_map, residual_variance, to_gauge_frame
from lib.synthetic import make_scene
from oracle import ba_oracle as O

AXES = ("x-right_z-forward", "x-up_z-forward")


# ---------------------------------------------------------------- parameter_map
@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("m", [2, 3, 7])
def test_default_map_is_the_gauge_strip(axis, m):
    col, n_free = parameter_map(m, axis)
    keep = np.setdiff1d(np.arange(9 * m), O.gauge_removed(axis))
    assert n_free == 9 * m - 7 and col.dtype == np.int32
    assert np.array_equal(np.nonzero(col >= 0)[0], keep)
    assert np.array_equal(col[keep], np.arange(9 * m - 7))
    assert (col[O.gauge_removed(axis)] == -1).all()


def test_named_forms_against_hand_written_maps():
    H = -1
    ax = "x-right_z-forward"  # gauge: 3..8 and 12
    cases = {
        (("hold", "intrinsics"),): [H, H, H, H, H, H, H, H, H, H, H, H, H, 0, 1, 2, 3, 4, H, H, H, 5, 6, 7, 8, 9, 10],
        (("hold", "f"),): [H, 0, 1, H, H, H, H, H, H, H, 2, 3, H, 4, 5, 6, 7, 8, H, 9, 10, 11, 12, 13, 14, 15, 16],
        (("hold", "u"),): [0, H, H, H, H, H, H, H, H, 1, H, H, H, 2, 3, 4, 5, 6, 7, H, H, 8, 9, 10, 11, 12, 13],
        (("hold", "t"),): [0, 1, 2, H, H, H, H, H, H, 3, 4, 5, H, H, H, 6, 7, 8, 9, 10, 11, H, H, H, 12, 13, 14],
        (("hold", "R"),): [0, 1, 2, H, H, H, H, H, H, 3, 4, 5, H, 6, 7, H, H, H, 8, 9, 10, 11, 12, 13, H, H, H],
        (("hold", "pose"),): [0, 1, 2, H, H, H, H, H, H, 3, 4, 5, H, H, H, H, H, H, 6, 7, 8, H, H, H, H, H, H],
        (("hold", ("t", "R")),): [0, 1, 2, H, H, H, H, H, H, 3, 4, 5, H, H, H, H, H, H, 6, 7, 8, H, H, H, H, H, H],
        (("hold", "cameras"),): [H] * 27,
        (("share", "intrinsics"),): [11, 12, 13, H, H, H, H, H, H, 11, 12, 13, H, 0, 1, 2, 3, 4, 11, 12, 13, 5, 6, 7, 8, 9, 10],
        (("share", "f"),): [17, 0, 1, H, H, H, H, H, H, 17, 2, 3, H, 4, 5, 6, 7, 8, 17, 9, 10, 11, 12, 13, 14, 15, 16],
        (("share", "u"),): [0, 14, 15, H, H, H, H, H, H, 1, 14, 15, H, 2, 3, 4, 5, 6, 7, 14, 15, 8, 9, 10, 11, 12, 13],
        (("share", "f"), ("hold", "u")): [11, H, H, H, H, H, H, H, H, 11, H, H, H, 0, 1, 2, 3, 4, 11, H, H, 5, 6, 7, 8, 9, 10],
        # cameras 0 and 2 are one body, camera 1 alone: its intrinsics stay ordinary unknowns
        (("share", "intrinsics"), ("share_groups", (4, 9, 4))): [14, 15, 16, H, H, H, H, H, H, 0, 1, 2, H, 3, 4, 5, 6, 7,
                                                                 14, 15, 16, 8, 9, 10, 11, 12, 13],
    }
    for args, want in cases.items():
        kw = {k: (np.array(v) if k == "share_groups" else v) for k, v in args}
        col, n_free = parameter_map(3, ax, **kw)
        assert col.tolist() == want, args
        assert n_free == max(want) + 1, args
    # x-up: camera 1's t_y (slot 13) is the gauge slot
    col, n_free = parameter_map(3, "x-up_z-forward", hold="intrinsics")
    assert col.tolist() == [H] * 12 + [0, H, 1, 2, 3, 4, H, H, H, 5, 6, 7, 8, 9, 10] and n_free == 11
    # mask form: True = held; the gauge slots are held whatever the mask says
    mask = np.zeros((3, 9), bool)
    mask[1, 0] = mask[2, 6:] = True
    col, n_free = parameter_map(3, ax, hold=mask)
    assert col.tolist() == [0, 1, 2, H, H, H, H, H, H, H, 3, 4, H, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, H, H, H] and n_free == 16
    # a group that is held as a whole in a shared slot is simply held
    mask = np.zeros((3, 9), bool)
    mask[:, 0] = True
    col, n_free = parameter_map(3, ax, hold=mask, share="intrinsics")
    assert (col[[0, 9, 18]] == -1).all() and col[1] == col[10] == col[19] == n_free - 2


def test_parameter_map_errors():
    with pytest.raises(ValueError, match="unknown name 'focal'"):
        parameter_map(3, AXES[0], hold="focal")
    with pytest.raises(ValueError, match="unknown name 't'"):
        parameter_map(3, AXES[0], share="t")
    with pytest.raises(ValueError, match="'f' is both held and shared"):
        parameter_map(3, AXES[0], hold="intrinsics", share="f")
    mask = np.zeros((3, 9), bool)
    mask[1, 0] = True
    with pytest.raises(ValueError, match="group 0: slot 'f' is held for some"):
        parameter_map(3, AXES[0], hold=mask, share="f")
    with pytest.raises(ValueError, match="hold"):
        parameter_map(3, AXES[0], hold=np.zeros((2, 9), bool))
    with pytest.raises(ValueError, match="share_groups"):
        parameter_map(3, AXES[0], share="f", share_groups=np.zeros(2, int))
    with pytest.raises(ValueError):
        parameter_map(3, "z-up", hold="f")


def test_adjuster_errors_come_before_any_device_work(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_mvba, "load_library", no_library)
    monkeypatch.setattr(_mvba, "device_count", no_library)
    sc = make_scene(20, 3, vis_p=1.0, project="numpy")
    args = (sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, sc.init_X, sc.init_K, sc.init_R, sc.init_t)
    K = sc.init_K.copy()
    K[:] = K[0]
    K[2, 0, 0] += 1.0
    K[1, 1, 2] -= 2.0
    for kw, msg in ((dict(hold="focal"), "unknown name"), (dict(hold="f", share="intrinsics"), "both held and shared"),
                    (dict(share_groups=np.zeros(3, int)), "share_groups without share")):
        with pytest.raises(ValueError, match=msg):
            BundleAdjuster.from_observations(*args, axis=sc.axis, **kw)
    bad = (sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, sc.init_X, K, sc.init_R, sc.init_t)
    with pytest.raises(ValueError, match="group 0: shared 'f' starts from different values"):
        BundleAdjuster.from_observations(*bad, axis=sc.axis, share="f")
    with pytest.raises(ValueError, match="group 5: shared 'v' starts from different values"):
        BundleAdjuster.from_observations(*bad, axis=sc.axis, share="u", share_groups=np.array([5, 5, 7]))
    x = np.zeros((sc.n_points, sc.n_images, 2))
    with pytest.raises(ValueError, match="starts from different values"):
        BundleAdjuster(x, sc.init_X, K, sc.init_R, sc.init_t, axis=sc.axis, share="intrinsics")


def test_binding_and_header_declare_the_entry_point():
    hdr = open(_mvba.os.path.join(_mvba.os.path.dirname(_mvba._HERE), "..", "include", "mvba.h")).read()
    assert "int mvba_set_parameter_map(mvba_handle *h, const int32_t *col, int32_t n_free);" in hdr
    assert "mvba_set_parameter_map" in _mvba.SIGNATURES


def test_residual_variance_takes_the_free_count():
    assert residual_variance(3.0, 100, 10, 4) == 3.0 / (200 - (30 + 29))
    assert residual_variance(3.0, 100, 10, 4, n_free=29) == residual_variance(3.0, 100, 10, 4)
    assert residual_variance(3.0, 100, 10, 4, n_free=17) == 3.0 / (200 - 47)
    assert residual_variance(3.0, 100, 10, 4, n_free=0) == 3.0 / 170
    with pytest.raises(ValueError, match="no redundancy"):
        residual_variance(1.0, 10, 10, 1, n_free=0)


# ---------------------------------------------------------------- the reference's step
def _engine(sc, shared_start=False):
    g = ConstrainedOracleEngine(sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis)
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    K = sc.init_K.copy()
    if shared_start:
        K[:] = K.mean(axis=0)
    g.set_params(X, K[:, 0, 0], K[:, :2, 2], t, R)
    return g


MAPS3 = [dict(hold="intrinsics"), dict(share="intrinsics"), dict(share="f", hold="u")]


@pytest.mark.parametrize("kw", MAPS3, ids=["hold_intr", "share_intr", "share_f_hold_u"])
def test_mapped_right_hand_side_is_the_gradient_in_the_reduced_unknowns(kw):
    """b = F^T E^-1 dP - dF, so P^T b = P^T (F^T E^-1 dP) - dE/dx with x the reduced unknowns (tied slots move together,
    omega through Rod(omega) R): the second term against central differences of the cost, step and tolerance of
    tests/test_robust_cpu.py's gradient test."""
    sc = make_scene(60, 5, 0.8, project="numpy")
    g = _engine(sc, shared_start=True)
    col, n_free = parameter_map(sc.n_images, sc.axis, **kw)
    g.set_parameter_map(col, n_free)
    g.linearize()
    g.try_step(1e-4)
    P = map_matrix(col, n_free)
    Y = np.einsum("oij,ojk->oik", g.Einv[g.pt], g.F)
    schur_b = O._segsum(g.cam, np.einsum("oji,oj->oi", Y, g.dP[g.pt]), g.m).reshape(-1)
    X0, f0_, u0, t0, R0 = g.get_params()

    def E_at(x):
        d = (P @ x).reshape(g.m, 9)
        Rn = np.stack([O.rodrigues(w) for w in d[:, 6:9]]) @ R0
        return O.cost(X0, f0_ + d[:, 0], u0 + d[:, 1:3], t0 + d[:, 3:6], Rn, 1.0, g.pt, g.cam, g.xy)

    scale = np.abs(g.dF).max()
    num = np.zeros(n_free)
    for j in range(n_free):
        members = np.nonzero(col == j)[0]
        h = 1e-4 * (max(1.0, abs(f0_[members[0] // 9])) if members[0] % 9 == 0 else 1.0)
        x = np.zeros(n_free)
        x[j] = h
        num[j] = (E_at(x) - E_at(-x)) / (2 * h)
    np.testing.assert_allclose(P.T @ schur_b - g.b, num, rtol=1e-5, atol=1e-7 * scale)
    # and the step: held slots exactly 0, tied slots exactly equal
    dxi = P @ g.dxi_red
    assert (dxi[col < 0] == 0).all()
    for j in range(n_free):
        assert len(set(dxi[col == j].tolist())) == 1


@pytest.mark.parametrize("axis", AXES)
def test_default_map_reproduces_the_oracle_bitwise(axis):
    sc = make_scene(60, 5, 0.8, project="numpy")
    args = (sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, axis)
    g, o = ConstrainedOracleEngine(*args), O.OracleEngine(*args)
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, axis)
    for e in (g, o):
        e.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    g.set_parameter_map(*parameter_map(sc.n_images, axis))
    for c in (1e-4, 1e-1):
        g.linearize(); o.linearize()
        assert g.try_step(c) == o.try_step(c)
        assert np.array_equal(g.dxi_red, o.dxi_red) and np.array_equal(g.dX, o.dX)
        g.commit(); o.commit()
    for a, b in zip(g.get_params(), o.get_params()):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- BundleAdjuster over the reference engine
@pytest.fixture(scope="module")
def runs():
    sc = make_scene(300, 8, 0.7, project="numpy")
    K = sc.init_K.copy()
    K[:] = K.mean(axis=0)  # one camera body: equal starting intrinsics
    out = {}
    for name, kw in (("free", {}), ("hold_intr", dict(hold="intrinsics")), ("share_intr", dict(share="intrinsics")),
                     ("share_f_hold_u", dict(share="f", hold="u")), ("hold_pose", dict(hold="pose")),
                     ("hold_all", dict(hold="cameras")),
                     ("groups", dict(share="intrinsics", share_groups=np.array([0, 0, 0, 1, 1, 0, 0, 0])))):
        ba = RefAdjuster.from_observations(sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, sc.init_X, K, sc.init_R,
                                           sc.init_t, axis=sc.axis, **kw)
        E0 = ba._engine.cost()
        X, Ko, R, t = ba.optimize(10.0, 1e-10, 30)
        E = O.cost(*(lambda Xg, Rg, tg: (Xg, Ko[:, 0, 0], Ko[:, :2, 2], tg, Rg))(*to_gauge_frame(X, R, t, sc.axis)), 1.0,
                   ba._engine.pt, ba._engine.cam, ba._engine.xy)
        out[name] = dict(ba=ba, E0=E0, E=E, X=X, K=Ko, R=R, t=t)
    return sc, K, out


def test_held_parameters_come_back_as_they_went_in(runs):
    sc, K, out = runs
    for name in ("hold_intr", "hold_all"):
        assert np.array_equal(out[name]["K"][:, 0, 0], K[:, 0, 0]) and np.array_equal(out[name]["K"][:, :2, 2], K[:, :2, 2])
    assert np.array_equal(out["share_f_hold_u"]["K"][:, :2, 2], K[:, :2, 2])
    for name in ("hold_pose", "hold_all"):  # held in the gauge frame: the way there and back costs rounding only
        np.testing.assert_allclose(out[name]["R"], sc.init_R, rtol=0, atol=1e-12)
        np.testing.assert_allclose(out[name]["t"], sc.init_t, rtol=0, atol=1e-12 * max(1.0, np.abs(sc.init_t).max()))
    assert not np.array_equal(out["hold_pose"]["K"], K) and not np.array_equal(out["hold_intr"]["t"], sc.init_t)


def test_tied_parameters_stay_equal_bit_for_bit(runs):
    _, K, out = runs
    Ko = out["share_intr"]["K"]
    for v in (Ko[:, 0, 0], Ko[:, 0, 2], Ko[:, 1, 2]):
        assert len(set(v.tolist())) == 1
    assert Ko[0, 0, 0] != K[0, 0, 0]
    assert len(set(out["share_f_hold_u"]["K"][:, 0, 0].tolist())) == 1
    Kg = out["groups"]["K"]
    for grp in ([0, 1, 2, 5, 6, 7], [3, 4]):
        for v in (Kg[grp, 0, 0], Kg[grp, 0, 2], Kg[grp, 1, 2]):
            assert len(set(v.tolist())) == 1
    assert Kg[0, 0, 0] != Kg[3, 0, 0]


def test_costs_fall_and_nest(runs):
    """hold intrinsics is a sub-model of share intrinsics (the shared value may stay), which is one of everything free:
    E_held >= E_shared >= E_free at convergence; likewise two groups lie between one group and free, and holding
    everything is above all."""
    _, _, out = runs
    for name, r in out.items():
        assert r["E"] < r["E0"], name
    E = {k: v["E"] for k, v in out.items()}
    assert E["hold_intr"] >= E["share_intr"] - 1e-12 and E["share_intr"] >= E["free"] - 1e-12
    assert E["share_intr"] >= E["groups"] - 1e-12 and E["groups"] >= E["free"] - 1e-12
    assert E["hold_intr"] >= E["share_f_hold_u"] - 1e-12
    assert E["hold_all"] >= E["hold_pose"] - 1e-12 and E["hold_all"] >= E["hold_intr"] - 1e-12
    assert out["hold_intr"]["ba"].n_free_camera_parameters == 9 * 8 - 7 - 24
    assert out["share_intr"]["ba"].n_free_camera_parameters == 9 * 8 - 7 - 24 + 3
    assert out["hold_all"]["ba"].n_free_camera_parameters == 0 and out["free"]["ba"].n_free_camera_parameters == 65


# ---------------------------------------------------------------- the trajectory cases of tests/test_gpu_constraints.py
@pytest.mark.parametrize("name,axis,args", [("linearize_60x7_xup", "x-up_z-forward", (10.0, 1e-8, 8)),
                                             ("linearize_60x7_xright", "x-right_z-forward", (10.0, 1e-8, 8)),
                                             ("visibility_300x12", "x-up_z-forward", (2.0, 1e-10, 10))])
@pytest.mark.parametrize("kw", MAPS3, ids=["hold_intr", "share_intr", "share_f_hold_u"])
def test_trajectory_cases_do_not_hang_on_a_tie(golden, name, axis, args, kw):
    """The GPU trajectory test asserts equal iteration and solve counts; that is only meaningful where no accept test
    E' > E falls within rounding.  Here: the reference, run again with A perturbed by 1e-13 relative (two seeds), keeps
    its counts on every case that test uses."""
    d = golden(name)
    vis = d["vis"] if "vis" in d.files else None
    K = d["init_K"].copy()
    K[:] = K.mean(axis=0)

    def run(seed):
        ba = RefAdjuster(d["x"], d["init_X"], K, d["init_R"], d["init_t"], visibility_index=vis, axis=axis, **kw)
        if seed is not None:
            rng, eng = np.random.default_rng(seed), ba._engine
            plain = eng.solve_reduced
            eng.solve_reduced = lambda A, b: plain(A * (1.0 + 1e-13 * rng.uniform(-1, 1, A.shape)), b)
        ba.optimize(*args, is_debug=True)
        return len(ba.get_log()), ba._engine.n_solves

    base = run(None)
    assert run(1) == base and run(2) == base
