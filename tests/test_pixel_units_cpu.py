"""The unit-twin method of tests/_pixel_cases.py on the CPU oracle: its premises hold (a pixel problem and its twin agree
after scaling, bit for bit at f0 = 512, within the existing bounds at f0 = 600, with equal LM solve counts), and it can
fail (an engine that drops or misplaces f0 is caught at 512 and 600 -- and passes at f0 = 1, which is the gap the GPU tests
of tests/test_gpu_pixel_units.py close).  The same for the robust and the constrained reference engines."""
import numpy as np
import pytest

from _constraints_ref import ConstrainedOracleEngine
from _pixel_cases import ORACLE_TWIN_DXI, assert_twin, dxi_bound, engine_outputs, make_engine, pixel_problem, to_twin_units
from _robust_ref import RobustOracleEngine
from lib.bundle_adjustment import lm_loop, parameter_map
from oracle import ba_oracle as O

# bit for bit on the oracle at a power of two; dxi and what follows it are not (NumPy's LU pivots by magnitude, which the
# scaling changes): those are held to the bounds of the f0 = 600 comparison at either f0
EXACT = ("cost", "residual", "JX", "JC", "E", "dP", "A", "b")
SHAPES = [(300, 8, 0.5), (900, 30, 0.2)]


def _twin_checks(cls, px, twin, D, f0, exact_keys=EXACT, setup=None, **kw):
    """The three checks: exact (at 512) / bounded (at 600) one step, and equal solve counts over six LM iterations."""
    a, b = make_engine(cls, px, **kw), make_engine(cls, twin, **{**kw, **({"loss_scale": kw["loss_scale"] / f0} if "loss_scale" in kw else {})})
    if setup:
        setup(a), setup(b)
    oa, ob = engine_outputs(a, 1e-4), engine_outputs(b, 1e-4)
    if f0 == 512.0:
        assert_twin({k: oa[k] for k in exact_keys}, {k: ob[k] for k in exact_keys}, D, exact=True)
    assert_twin(oa, ob, D, exact=False)
    a.n_solves = b.n_solves = 0
    Ea, Eb = lm_loop(a, 2.0, -1.0, 6, verbose=False), lm_loop(b, 2.0, -1.0, 6, verbose=False)
    assert a.n_solves == b.n_solves
    assert Ea == pytest.approx(Eb, rel=1e-9)
    return a, b


@pytest.mark.parametrize("f0", [512.0, 600.0])
@pytest.mark.parametrize("n,m,p", SHAPES)
def test_oracle_pixel_problem_equals_its_twin(n, m, p, f0):
    px, twin, D = pixel_problem(n, m, p, f0)
    assert (px[9] != px[9][:, ::-1]).all() and px[8].min() > 0.9 * f0  # u != v, f ~ f0
    _twin_checks(O.OracleEngine, px, twin, D, f0)


@pytest.mark.parametrize("shape,loss", list(ORACLE_TWIN_DXI), ids=lambda v: str(v).replace(" ", ""))
def test_recorded_oracle_twin_differences(shape, loss):
    """The cases where the oracle's own solve at f0 = 600 is further from its twin's than the existing 1e-9 bound on dxi: the
    figures recorded in _pixel_cases.ORACLE_TWIN_DXI (from which the GPU tests set their bound on those cases) are measured
    here -- not exceeded, and not more than twice what is measured.  Everything up to the solve agrees within the existing
    bounds, so the difference is the solve's."""
    recorded = ORACLE_TWIN_DXI[(shape, loss)]
    robust = loss != "squared"
    px, twin, D = pixel_problem(*shape, 600.0, outlier_frac=0.08 if robust else 0.0)
    scale_px, c = 2.0, (1e-3 if robust else 1e-4)  # (the GPU test's loss scale and damping)
    if robust:
        a = make_engine(RobustOracleEngine, px, loss=loss, loss_scale=scale_px)
        b = make_engine(RobustOracleEngine, twin, loss=loss, loss_scale=scale_px / 600.0)
    else:
        a, b = make_engine(O.OracleEngine, px), make_engine(O.OracleEngine, twin)
    oa, ob = engine_outputs(a, c), engine_outputs(b, c)
    assert_twin({k: oa[k] for k in EXACT}, {k: ob[k] for k in EXACT}, D, exact=False)
    got = np.abs(to_twin_units("dxi", oa["dxi"], D) - ob["dxi"]).max() / np.abs(ob["dxi"]).max()
    print(f"oracle at f0 = 600 against its twin, {shape} {loss}: |ddxi| / max|dxi| = {got:.3e} (recorded {recorded:g}; existing bound 1e-9)")
    assert 1e-9 < got <= recorded <= 2.0 * got


@pytest.mark.parametrize("shape", [(3000, 12, 0.5), (3000, 30, 0.3)], ids=lambda v: str(v).replace(" ", ""))
def test_lane_form_shapes_need_no_recorded_oracle_twin_difference(shape):
    """The shapes on which tests/test_gpu_pixel_units.py and tests/test_gpu_lanes_sequence.py run the lane-form engines have no
    entry in _pixel_cases.ORACLE_TWIN_DXI: the f0 = 600 oracle lies within the existing 1e-9 of its own twin there (1.18e-10 and
    4.0e-11 of max|dxi| when this test was written), so dxi_bound() is the existing bound and the premise is re-measured here."""
    assert (shape, "squared") not in ORACLE_TWIN_DXI and dxi_bound(shape) == 1e-9
    px, twin, D = pixel_problem(*shape, 600.0)
    oa, ob = engine_outputs(make_engine(O.OracleEngine, px), 1e-4), engine_outputs(make_engine(O.OracleEngine, twin), 1e-4)
    assert_twin({k: oa[k] for k in EXACT}, {k: ob[k] for k in EXACT}, D, exact=False)
    got = np.abs(to_twin_units("dxi", oa["dxi"], D) - ob["dxi"]).max() / np.abs(ob["dxi"]).max()
    print(f"oracle at f0 = 600 against its twin, {shape}: |ddxi| / max|dxi| = {got:.3e} (bound 1e-9)")
    assert got <= 1e-9


class _Mutant(O.OracleEngine):
    """An oracle whose camera Jacobian mishandles f0, the way a kernel could:
    "uv_ignores_f0"   the (u, v) columns are 1 where they are 1 / f0 (f0 dropped on one branch);
    "f_unscaled_cam2" camera 2's f column is that of the unit problem (f0 applied once too often for one camera)."""

    def __init__(self, *a, mutation, **kw):
        super().__init__(*a, **kw)
        self.mutation = mutation

    def linearize(self):
        e, JX, JC = O.jacobians(self.X, self.f, self.u, self.t, self.R, self.f0, self.pt, self.cam, self.xy)
        if self.mutation == "uv_ignores_f0":
            JC[:, 0, 1] *= self.f0
            JC[:, 1, 2] *= self.f0
        else:
            JC[self.cam == 2, :, 0] *= self.f0
        self.e, self.JX, self.JC = e, JX, JC
        self.dP = 2.0 * O._segsum(self.pt, np.einsum("ori,or->oi", JX, e), self.n)
        self.dF = 2.0 * O._segsum(self.cam, np.einsum("ori,or->oi", JC, e), self.m)
        self.E = 2.0 * O._segsum(self.pt, np.einsum("ori,orj->oij", JX, JX), self.n)
        self.F = 2.0 * np.einsum("ori,orj->oij", JX, JC)
        self.G = 2.0 * O._segsum(self.cam, np.einsum("ori,orj->oij", JC, JC), self.m)


@pytest.mark.parametrize("mutation", ["uv_ignores_f0", "f_unscaled_cam2"])
def test_the_method_catches_a_misplaced_f0_and_f0_equal_one_does_not(mutation):
    n, m, p = SHAPES[0]
    for f0 in (512.0, 600.0):
        px, twin, D = pixel_problem(n, m, p, f0)
        good = engine_outputs(make_engine(O.OracleEngine, twin), 1e-4)
        bad = engine_outputs(make_engine(_Mutant, px, mutation=mutation), 1e-4)
        for keys in (("JC",), ("A",), ("b",), ("dxi",), ("dX", "trial_cost")):  # each on its own: the mutation shows in every one
            with pytest.raises(AssertionError):
                assert_twin({k: bad[k] for k in keys}, {k: good[k] for k in keys}, D, exact=False)
        if f0 == 512.0:
            with pytest.raises(AssertionError):
                assert_twin({k: bad[k] for k in EXACT}, {k: good[k] for k in EXACT}, D, exact=True)
        assert_twin({k: bad[k] for k in ("cost", "residual", "JX", "E", "dP")},
                    {k: good[k] for k in ("cost", "residual", "JX", "E", "dP")}, D, exact=(f0 == 512.0))  # untouched by it
    # the gap: at f0 = 1 the mutants are the oracle, bit for bit -- what every numerical BA test used before
    px, twin, D = pixel_problem(n, m, p, 1.0)
    assert (D == 1.0).all() and all(np.array_equal(a, b) for a, b in zip(px[4:], twin[4:]) if not isinstance(a, str))
    good = engine_outputs(make_engine(O.OracleEngine, twin), 1e-4)
    bad = engine_outputs(make_engine(_Mutant, px, mutation=mutation), 1e-4)
    assert_twin(bad, good, D, exact=True)


@pytest.mark.parametrize("f0", [512.0, 600.0])
@pytest.mark.parametrize("loss,scale_px", [("huber", 3.0), ("cauchy", 2.0)])
def test_robust_oracle_with_the_loss_scale_in_pixels(loss, scale_px, f0):
    px, twin, D = pixel_problem(300, 8, 0.5, f0, outlier_frac=0.08)
    a, b = _twin_checks(RobustOracleEngine, px, twin, D, f0, exact_keys=EXACT + ("weight",), loss=loss, loss_scale=scale_px)
    assert a.loss_b == b.loss_b == (scale_px / f0) ** 2  # b = (delta / f0)^2 is the same number in both
    a.linearize()
    assert a.w.min() < 0.5 and (a.w == 1.0).sum() > 0 if loss == "huber" else a.w.min() < 0.5  # both branches of the loss


@pytest.mark.parametrize("f0", [512.0, 600.0])
@pytest.mark.parametrize("kind", ["hold_intr", "share_intr"])
def test_constrained_oracle(kind, f0):
    n, m, p = 300, 8, 0.5
    px, twin, D = pixel_problem(n, m, p, f0, one_body=True)
    col, n_free = parameter_map(m, px[6], **({"hold": "intrinsics"} if kind == "hold_intr" else {"share": "intrinsics"}))
    a, b = _twin_checks(ConstrainedOracleEngine, px, twin, D, f0, setup=lambda e: e.set_parameter_map(col, n_free))
    fa, ua = a.get_params()[1:3]
    fb, ub = b.get_params()[1:3]
    if kind == "hold_intr":
        assert np.array_equal(fa, px[8]) and np.array_equal(ua, px[9])
    else:
        assert len(set(fa.tolist())) == 1 and len(set(map(tuple, ua.tolist()))) == 1 and not np.array_equal(fa, px[8])
    np.testing.assert_allclose(fa / f0, fb, rtol=0, atol=1e-9)
    np.testing.assert_allclose(ua / f0, ub, rtol=0, atol=1e-9)
