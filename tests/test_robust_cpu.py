"""Robust losses on the host: the loss table, the reference's weighted gradient, the Huber limit and argument validation
(no GPU needed)."""
import numpy as np
import pytest

from _robust_ref import RobustOracleEngine, inject_outliers, rho, robust_cost, weight
from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster, lm_loop, loss_weights
from lib.synthetic import make_scene
from oracle import ba_oracle as O


def test_rho_and_weight_follow_the_table():
    b = 0.25
    s = np.array([0.0, 0.1, 0.25, 0.3, 4.0, 100.0])
    np.testing.assert_allclose(rho(s, b, "squared"), s)
    np.testing.assert_allclose(weight(s, b, "squared"), 1.0)
    hub = [v if v <= b else 2 * np.sqrt(b * v) - b for v in s]
    np.testing.assert_allclose(rho(s, b, "huber"), hub, rtol=1e-15)
    np.testing.assert_allclose(weight(s, b, "huber"), [1.0 if v <= b else np.sqrt(b / v) for v in s], rtol=1e-15)
    np.testing.assert_allclose(rho(s, b, "cauchy"), b * np.log1p(s / b), rtol=1e-15)
    np.testing.assert_allclose(weight(s, b, "cauchy"), 1 / (1 + s / b), rtol=1e-15)
    # w = rho'(s): central differences away from Huber's kink
    for loss in ("huber", "cauchy"):
        for v in (0.1, 0.7, 9.0):
            h = 1e-6 * v
            d = (rho(v + h, b, loss) - rho(v - h, b, loss)) / (2 * h)
            assert d == pytest.approx(float(weight(v, b, loss)), rel=1e-7)
    # continuity of Huber at s = b
    assert float(rho(b * (1 + 1e-12), b, "huber")) == pytest.approx(b, rel=1e-11)


def test_host_weights_match_the_reference():
    rng = np.random.default_rng(1)
    e = rng.normal(scale=3.0, size=(50, 2))
    f0 = 2.0
    for loss, scale in (("squared", None), ("huber", 1.5), ("cauchy", 0.7)):
        s = ((e / f0) ** 2).sum(axis=1)
        b = (scale / f0) ** 2 if scale else 1.0
        np.testing.assert_allclose(loss_weights(e, f0, loss, scale), weight(s, b, loss), rtol=1e-15)


def _robust_pair(loss, scale, frac=0.08, seed=3):
    sc = make_scene(60, 6, vis_p=0.7, seed=seed, project="numpy")
    xy, _ = inject_outliers(sc.xy, frac, 20.0, 100.0, seed=seed)
    g = RobustOracleEngine(sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, xy, 1.0, sc.axis, loss=loss, loss_scale=scale)
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    g.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    return g, sc, xy


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_weighted_gradient_is_the_gradient_of_the_robust_cost(loss):
    """2 J^T W e (the reference's dP, dF) against a central difference of E = sum rho over points and cameras."""
    g, sc, xy = _robust_pair(loss, 2.0)
    g.linearize()
    X0, f0_, u0, t0, R0 = g.get_params()

    def E_at(X, f, u, t, R):
        return robust_cost(X, f, u, t, R, 1.0, g.pt, g.cam, g.xy, g.loss_b, loss)

    for a in (0, 7, 31):
        for i in range(3):
            h = 1e-4 * max(1.0, abs(X0[a, i]))  # (E ~ 5e3: a smaller step drowns in rounding)
            Xp, Xm = X0.copy(), X0.copy()
            Xp[a, i] += h
            Xm[a, i] -= h
            num = (E_at(Xp, f0_, u0, t0, R0) - E_at(Xm, f0_, u0, t0, R0)) / (2 * h)
            assert g.dP[a, i] == pytest.approx(num, rel=1e-5, abs=1e-7 * abs(g.dP).max())
    for k in (1, 4):
        h = 1e-4 * max(1.0, abs(f0_[k]))
        fp, fm = f0_.copy(), f0_.copy()
        fp[k] += h
        fm[k] -= h
        num = (E_at(X0, fp, u0, t0, R0) - E_at(X0, fm, u0, t0, R0)) / (2 * h)
        assert g.dF[k, 0] == pytest.approx(num, rel=1e-5, abs=1e-7 * abs(g.dF).max())
        for j in range(2):
            up, um = u0.copy(), u0.copy()
            up[k, j] += 1e-4
            um[k, j] -= 1e-4
            num = (E_at(X0, f0_, up, t0, R0) - E_at(X0, f0_, um, t0, R0)) / 2e-4
            assert g.dF[k, 1 + j] == pytest.approx(num, rel=1e-5, abs=1e-7 * abs(g.dF).max())


def test_huber_above_every_residual_is_the_squared_trajectory():
    sc = make_scene(80, 6, vis_p=0.8, project="numpy")
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    args = (sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis)
    sq = O.OracleEngine(*args)
    sq.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    e = O.residuals(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R, 1.0, sq.pt, sq.cam, sq.xy)
    hub = RobustOracleEngine(*args, loss="huber", loss_scale=1e3 * (1 + np.abs(e).max()))
    hub.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    E1 = lm_loop(sq, 2.0, -1.0, 6, verbose=False)
    E2 = lm_loop(hub, 2.0, -1.0, 6, verbose=False)
    assert E1 == E2 and sq.n_solves == hub.n_solves
    for a, b in zip(sq.get_params(), hub.get_params()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("loss,scale", [("tukey", 1.0), ("huber", None), ("cauchy", 0.0), ("huber", -2.0),
                                         ("cauchy", float("nan")), ("huber", float("inf")), (1, 1.0), ("huber", "x")])
def test_bad_loss_arguments_raise_before_any_library_call(monkeypatch, loss, scale):
    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_mvba, "load_library", no_library)
    monkeypatch.setattr(_mvba, "device_count", no_library)
    sc = make_scene(20, 3, vis_p=1.0, project="numpy")
    with pytest.raises(ValueError):
        _mvba.HipEngine(sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, 1.0, sc.axis, loss=loss, loss_scale=scale)
    with pytest.raises(ValueError):
        BundleAdjuster.from_observations(sc.n_points, sc.n_images, sc.pt_ptr, sc.cam_idx, sc.xy, sc.init_X, sc.init_K,
                                         sc.init_R, sc.init_t, axis=sc.axis, loss=loss, loss_scale=scale)
    x = np.zeros((sc.n_points, sc.n_images, 2))
    with pytest.raises(ValueError):
        BundleAdjuster(x, sc.init_X, sc.init_K, sc.init_R, sc.init_t, axis=sc.axis, loss=loss, loss_scale=scale)


def test_check_loss_codes_match_the_header():
    hdr = open(_mvba.os.path.join(_mvba.os.path.dirname(_mvba._HERE), "..", "include", "mvba.h")).read()
    for name, code in _mvba.LOSSES.items():
        assert f"#define MVBA_LOSS_{name.upper()} {code}" in hdr
    assert _mvba.check_loss("squared", None) == (0, 0.0)
    assert _mvba.check_loss("huber", 3) == (1, 3.0)
    assert _mvba.check_loss("cauchy", 0.5) == (2, 0.5)
