"""The BA engine away from f0 = 1: problems in pixel units (f ~ f0, principal points near (320, 240)) in every Schur form,
with the robust losses, parameter maps, covariances and through the public adjuster (tests/_pixel_cases.py).

Two comparisons, both in the units of the problem's unit twin (xy / f0, f0 = 1, f / f0, u / f0 -- the same problem):
  f0 = 512  the pixel engine against a second HIP engine on the twin.  Scaling by a power of two is exact and both engines
            run the same kernels in the same order (the Cholesky solve has no pivoting), so every output agrees BIT FOR BIT
            after the scaling; a missing, doubled or misplaced f0 breaks that grossly.  No tolerance is involved.
  f0 = 600  the pixel engine against the oracle with f0 = 600 (itself pinned to the reference at f0 = 600 by
            tests/test_oracle_golden.py), with the bounds of the existing test of each quantity on the column-scaled values:
            this pins the convention and shows that nothing relies on exactness.

The one-lane-per-item engines (rows "lanes", "lanes_full": k_schur_lanes_compact with the compact K1, k_schur_lanes) take f0 in
one place, jc_sign(i, cu) on the rows and columns of the 81 accumulators and cs * cs on the damping diagonal; at 512 they are
bitwise like every other form: the omega rows come from J_X, X_a and t, none of which scale, and cu, rs, cs are powers of two.

Left out on purpose: the indefinite-system shapes that take the LU rescue.  Partial pivoting compares magnitudes across
columns, so it is not covariant under the column scaling D and neither comparison applies to it."""
import contextlib
import functools
import io

import numpy as np
import pytest

from _constraints_ref import ConstrainedOracleEngine, map_matrix
from _covariance_ref import point_blocks, schur_covariance
from _parity_checks import check_one_step
from _pixel_cases import assert_twin, dxi_bound, engine_outputs, make_engine, pixel_problem, to_twin_units
from _robust_ref import RobustOracleEngine
from lib.bundle_adjustment import BundleAdjuster, intrinsics_from, lm_loop, parameter_map
from oracle import ba_oracle as O

pytestmark = pytest.mark.gpu

# the smallest shapes the suite already uses to reach each form: (id, (n, m, p), environment, schur_info()["kernel"])
FORMS = [
    ("pairs", (1500, 12, 0.4), {"MVBA_SCHUR": "pairs"}, "pairs"),
    ("pairs_big", (900, 9, 0.5), {"MVBA_SCHUR": "pairs", "MVBA_FORCE_BIG": "1"}, "pairs"),  # 64-bit offsets
    ("slots", (3000, 14, 0.5), {"MVBA_SCHUR": "slots"}, "slots"),
    ("dense_full", (300, 10, 1.0), {"MVBA_SCHUR": "dense"}, "dense"),
    ("dense_table", (400, 14, 0.8), {"MVBA_SCHUR": "dense"}, "dense"),  # missing observations: the table form
    ("gcam", (3000, 647, 0.04), {}, "pairs"),  # camera tables in device memory
    ("deg70", (90, 70, 1.0), {}, None),  # 70 observations per point > one 64-lane tile
    # one lane per item (k_schur_lanes_compact / k_schur_lanes): "slots" with step width 64, the record in LANE_RECORD;
    # three waves of 64 lists per range, the second off-diagonal wave with 2 of its 64 lists
    ("lanes", (3000, 12, 0.5), {"MVBA_SCHUR": "lanes"}, "slots"),
    ("lanes_full", (3000, 12, 0.5), {"MVBA_SCHUR": "lanes", "MVBA_REC": "full"}, "slots"),
]
FORM = {f[0]: f for f in FORMS}
IDS = [f[0] for f in FORMS]
LANE_RECORD = {"lanes": "compact", "lanes_full": "full"}  # the rows that must run the lane form, and on which record
LANES_ENV = FORM["lanes"][2]


@functools.lru_cache(maxsize=None)
def _problem(n, m, p, f0, **kw):
    """pixel_problem, built once per case and shared (the engines copy what they are given)."""
    return pixel_problem(n, m, p, f0, **kw)


def _hip(prob, **kw):
    from lib._mvba import HipEngine

    return make_engine(HipEngine, prob, **kw)


def _set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _assert_form(name, kernel, *engines):
    """Every engine runs the form the row names; a lane row that fell back to k_schur_slots (step width 21), to the unit form
    or to the other record fails here.  Returns the text the tests print."""
    for eng in engines:
        info = eng.schur_info()
        if kernel:
            assert info["kernel"] == kernel, info
        if name in LANE_RECORD:
            assert info["step_width"] == 64 and info["record"] == LANE_RECORD[name], info
    return f"form {info['kernel']}, step width {info['step_width']}, record {info['record']}"


def _close(a, b, tol, what, scale=None):
    """max|a - b| <= tol x scale, scale = max|b| unless given; the measured figure printed beside the bound."""
    scale = max(np.abs(b).max(), 1e-300) if scale is None else scale
    err = np.abs(np.asarray(a) - np.asarray(b)).max()
    print(f"  {what}: max|diff| / max = {err / scale:.3e} (bound {tol:g})")
    assert err <= tol * scale, (what, err, scale)


def _final_state(eng):
    eng.n_solves = 0
    with contextlib.redirect_stdout(io.StringIO()):
        lm_loop(eng, 2.0, -1.0, 5, verbose=False)
    out = dict(zip(("X", "f", "u", "t", "R"), eng.get_params()))
    out["n_solves"] = eng.n_solves
    out["lu_fallback"] = int(eng.stats()["counts"]["lu_fallback"])
    return out


# ---------------------------------------------------------------- every Schur form
@pytest.mark.parametrize("name,shape,env,kernel", FORMS, ids=IDS)
def test_twin_at_512_is_bitwise_in_every_form(monkeypatch, name, shape, env, kernel):
    """cost, residual, JX, JC, E, dP, A_full, b_full, dxi, dX, the trial state and cost and residuals() of one linearisation
    and one trial at c = 1e-4, then five LM iterations: equal solve counts, no LU rescue, bitwise equal final state."""
    _set_env(monkeypatch, env)
    px, twin, D = _problem(*shape, 512.0)
    a, b = _hip(px), _hip(twin)
    print(f"{name} {shape} f0 = 512, {_assert_form(name, kernel, a, b)}")
    assert_twin(engine_outputs(a, 1e-4), engine_outputs(b, 1e-4), D, exact=True)
    fa, fb = _final_state(a), _final_state(b)
    assert fa["lu_fallback"] == 0 and fb["lu_fallback"] == 0
    assert_twin(fa, fb, D, exact=True)


@pytest.mark.parametrize("name,shape,env,kernel", FORMS, ids=IDS)
def test_oracle_at_600_in_every_form(monkeypatch, name, shape, env, kernel):
    """_parity_checks.check_one_step against OracleEngine(..., 600.0, ...) with its existing bounds on the column-scaled values."""
    _set_env(monkeypatch, env)
    px, _, D = _problem(*shape, 600.0)
    eng = _hip(px)
    print(f"{name} {shape} f0 = 600, {_assert_form(name, kernel, eng)}")
    # (647 cameras and 90 x 70: the ORACLE's LU solve of the unscaled system is 1.4e-9 / 2.4e-9 from its own twin's -- measured on
    # the CPU, _pixel_cases.ORACLE_TWIN_DXI; the bound on dxi is MARGIN times that there, the existing 1e-9 everywhere else)
    check_one_step(eng, make_engine(O.OracleEngine, px), 1e-4, col_scale=D, dxi_tol=dxi_bound(shape))
    assert eng.stats()["counts"]["lu_fallback"] == 0


# ---------------------------------------------------------------- the reference's own numbers at f0 = 600
def test_golden_in_pixel_units(golden):
    """linearize_60x7_px (the reference with f0 = 600): one step against the oracle, column-scaled; the reference's own trial
    cost; the 8-iteration trajectory with the bounds of test_full_trajectory_vs_reference (E_log 1e-9 relative, outputs 1e-9,
    K's f and u in units of f0 as everywhere in this file), and K[2, 2] = f0 in the output."""
    d = golden("linearize_60x7_px")
    axis, f0, vis = "x-up_z-forward", 600.0, d["vis"]
    n, m = d["x"].shape[:2]
    D = np.ones((m, 9))
    D[:, :3] = f0
    ba = BundleAdjuster(d["x"], d["init_X"], d["init_K"], d["init_R"], d["init_t"], f0=f0, visibility_index=vis, axis=axis)
    pt_ptr, cam, xy = O.dense_to_observations(d["x"], vis)
    g = O.OracleEngine(n, m, pt_ptr, cam, xy, f0, axis)
    X, R, t = O.normalize_scene(d["init_X"], d["init_R"], d["init_t"], axis)
    g.set_params(X, d["init_K"][:, 0, 0], d["init_K"][:, :2, 2], t, R)
    E1 = check_one_step(ba._engine, g, float(d["c"]), col_scale=D.reshape(-1))
    print(f"  trial cost vs the reference's: rel. {abs(E1 - float(d['E1'])) / float(d['E1']):.3e} (bound 1e-9)")
    assert E1 == pytest.approx(float(d["E1"]), rel=1e-9)
    ba = BundleAdjuster(d["x"], d["init_X"], d["init_K"], d["init_R"], d["init_t"], f0=f0, visibility_index=vis, axis=axis)
    with contextlib.redirect_stdout(io.StringIO()):
        X, K, R, t = ba.optimize(10.0, 1e-8, 8, is_debug=True)
    E = np.array([e["reprojection_error"] for e in ba.get_log()])
    n_obs = ba._engine.n_obs
    assert abs(np.sqrt(E[-1] / n_obs) - np.sqrt(d["E_log"][-1] / n_obs)) < 1e-9
    assert len(E) == len(d["E_log"])
    assert ba._engine.n_solves == int(d["n_solves"])
    print(f"  E_log rel. {np.abs(E / d['E_log'] - 1).max():.3e} (1e-9), X {np.abs(X - d['out_X']).max():.3e}, K / f0 "
          f"{np.abs(K - d['out_K']).max() / f0:.3e}, R {np.abs(R - d['out_R']).max():.3e}, t {np.abs(t - d['out_t']).max():.3e} (1e-9)")
    np.testing.assert_allclose(E, d["E_log"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(X, d["out_X"], rtol=0, atol=1e-9)
    assert (K[:, 2, 2] == f0).all()
    np.testing.assert_allclose(K / f0, d["out_K"] / f0, rtol=0, atol=1e-9)
    np.testing.assert_allclose(R, d["out_R"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(t, d["out_t"], rtol=0, atol=1e-9)


# ---------------------------------------------------------------- robust losses, the scale in pixels
@pytest.mark.parametrize("loss,scale_px", [("huber", 3.0), ("cauchy", 2.0)])
@pytest.mark.parametrize("name", ["pairs", "dense_table", "gcam"])
def test_robust_losses_with_the_scale_in_pixels(monkeypatch, name, loss, scale_px):
    """b = (delta / f0)^2 and the sqrt(w) / f0 columns: the twin at 512 bit for bit, the weights included; at 600 the
    comparisons of tests/test_gpu_robust.py::_check_step against RobustOracleEngine with the same bounds, column-scaled; and
    residuals() = f0 e."""
    _, shape, env, kernel = FORM[name]
    _set_env(monkeypatch, env)
    px, twin, D = _problem(*shape, 512.0, outlier_frac=0.08)
    a, b = _hip(px, loss=loss, loss_scale=scale_px), _hip(twin, loss=loss, loss_scale=scale_px / 512.0)
    assert a.schur_info()["kernel"] == kernel
    print(f"{name} {shape} {loss} f0 = 512")
    oa, ob = engine_outputs(a, 1e-3), engine_outputs(b, 1e-3)
    assert oa["weight"].min() ** 2 < 0.5 and "weight" in ob  # the outliers are down-weighted
    assert_twin(oa, ob, D, exact=True)
    del a, b, oa, ob
    # f0 = 600 against the reference
    px, _, D = _problem(*shape, 600.0, outlier_frac=0.08)
    f0, m = 600.0, shape[1]
    eng, g = _hip(px, loss=loss, loss_scale=scale_px), make_engine(RobustOracleEngine, px, loss=loss, loss_scale=scale_px)
    print(f"{name} {shape} {loss} f0 = 600")
    _close(eng.cost(), g.cost(), 1e-12, "cost")
    _close(eng.residuals(), f0 * O.residuals(g.X, g.f, g.u, g.t, g.R, f0, g.pt, g.cam, g.xy), 1e-12, "residuals()")
    eng.linearize()
    g.linearize()
    n_obs, d9, DD = g.xy.shape[0], D[:9], np.outer(D, D)
    _close(eng.debug_read("weight") ** 2, g.w, 1e-12, "weight")
    _close(eng.debug_read("residual").reshape(n_obs, 2), g.e, 1e-11, "residual")
    _close(eng.debug_read("JX").reshape(n_obs, 2, 3), g.JX, 1e-11, "JX")
    _close(eng.debug_read("JC").reshape(n_obs, 2, 9) * d9, g.JC * d9, 1e-11, "JC D")
    E1 = eng.try_step(1e-3)
    A, bb = g.reduced_system(1e-3)
    E1o = g.try_step(1e-3)
    _close(eng.debug_read("A_full").reshape(9 * m, 9 * m) * DD, A * DD, 1e-10, "D A_full D")
    _close(eng.debug_read("b_full") * D, bb * D, 1e-10, "D b_full")
    _close(eng.debug_read("dX").reshape(-1, 3), g.dX, 1e-9, "dX")
    _close(eng.debug_read("trial_X").reshape(-1, 3), g.tX, 1e-10, "trial_X")
    tc = eng.debug_read("trial_cam").reshape(m, 15)
    # trial f, u = state + dxi: _check_step's 1e-10 of the largest, unless the oracle's own solve is recorded as further than that
    # from its twin's on this case (_pixel_cases.ORACLE_TWIN_DXI) -- then MARGIN times the recorded figure, of max|dxi|
    tol_fu, scale_fu = 1e-10, None
    if dxi_bound(shape, loss) > 1e-9:
        tol_fu, scale_fu = dxi_bound(shape, loss), np.abs(g.dxi_red / D[g.keep]).max()
    _close(tc[:, 0] / f0, g.tf / f0, tol_fu, "trial f / f0", scale_fu)
    _close(tc[:, 1:3] / f0, g.tu / f0, tol_fu, "trial u / f0", scale_fu)
    _close(tc[:, 3:6], g.tt, 1e-9, "trial t")
    print(f"  trial cost rel. {abs(E1 - E1o) / E1o:.3e} (bound 1e-9)")
    assert E1 == pytest.approx(E1o, rel=1e-9)
    assert g.w.min() < 0.5


# ---------------------------------------------------------------- parameter maps
def _map(kind, m, axis):
    if kind == "random_mask":
        return parameter_map(m, axis, hold=np.random.default_rng(5).random((m, 9)) < 0.4)
    return parameter_map(m, axis, **({"hold": "intrinsics"} if kind == "hold_intr" else {"share": "intrinsics"}))


KINDS = ["hold_intr", "share_intr", "random_mask"]


@pytest.mark.parametrize("kind", KINDS)
def test_parameter_maps(kind):
    """The mapped solve: dxi, dX and the trial state bit for bit against the twin at 512; at 600 against
    ConstrainedOracleEngine with the bounds of tests/test_gpu_constraints.py::_check_step, dxi in the twin's units."""
    _check_parameter_maps(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_parameter_maps_in_the_lane_form(monkeypatch, kind):
    """test_parameter_maps once more, same shape and bounds, with every engine in the lane form on the compact record
    (k_schur_lanes_compact feeds the mapped gather): shared intrinsics and a random hold mask as well as held intrinsics."""
    _set_env(monkeypatch, LANES_ENV)
    _check_parameter_maps(kind, form="lanes")


def _check_parameter_maps(kind, form=None):
    shape = (2000, 30, 0.3)
    m = shape[1]
    keys = ("dxi", "dX", "trial_X", "trial_cam", "trial_cost")
    px, twin, D = _problem(*shape, 512.0, one_body=True)
    col, n_free = _map(kind, m, px[6])
    a, b = _hip(px), _hip(twin)
    a.set_parameter_map(col, n_free), b.set_parameter_map(col, n_free)
    print(f"{kind} {shape} f0 = 512, n_free {n_free}, {_assert_form(form, None, a, b)}")
    assert_twin(engine_outputs(a, 1e-4, keys), engine_outputs(b, 1e-4, keys), D, exact=True)
    assert a.stats()["counts"]["lu_fallback"] == 0 and b.stats()["counts"]["lu_fallback"] == 0
    del a, b
    px, _, D = _problem(*shape, 600.0, one_body=True)
    f0 = 600.0
    eng, ref = _hip(px), make_engine(ConstrainedOracleEngine, px)
    _assert_form(form, None, eng)
    eng.set_parameter_map(col, n_free), ref.set_parameter_map(col, n_free)
    eng.linearize(), ref.linearize()
    E, Eo = eng.try_step(1e-4), ref.try_step(1e-4)
    dxi_ref = (map_matrix(col, n_free) @ ref.dxi_red) / D
    raw = eng.debug_read("dxi")
    dxi = raw / D
    print(f"{kind} {shape} f0 = 600: max|dxi - ref| / max|dxi| (twin's units) = {np.abs(dxi - dxi_ref).max() / np.abs(dxi_ref).max():.3e} "
          f"(bound 1e-9), |E - Eo| / Eo = {abs(E - Eo) / Eo:.3e} (bound 1e-12)")
    np.testing.assert_allclose(dxi, dxi_ref, rtol=0, atol=1e-9 * np.abs(dxi_ref).max())
    assert (raw[col < 0] == 0).all()
    for j in np.unique(col[col >= 0]):
        assert len(set(raw[col == j].tolist())) == 1
    np.testing.assert_allclose(eng.debug_read("dX").reshape(-1, 3), ref.dX, rtol=0, atol=1e-9 * np.abs(ref.dX).max())
    np.testing.assert_allclose(eng.debug_read("trial_X").reshape(-1, 3), ref.tX, rtol=0, atol=1e-10)
    tc = eng.debug_read("trial_cam").reshape(m, 15)
    np.testing.assert_allclose(tc[:, 0] / f0, ref.tf / f0, atol=1e-10)
    np.testing.assert_allclose(tc[:, 1:3] / f0, ref.tu / f0, atol=1e-10)
    np.testing.assert_allclose(tc[:, 3:6], ref.tt, atol=1e-10)
    np.testing.assert_allclose(tc[:, 6:].reshape(-1, 3, 3), ref.tR, atol=1e-10)
    assert E == pytest.approx(Eo, rel=1e-12)
    assert eng.stats()["counts"]["lu_fallback"] == 0


# ---------------------------------------------------------------- the compact record's other reader
def test_debug_reads_of_the_compact_record_at_600(monkeypatch):
    """tests/test_gpu_compact_record.py::test_debug_reads_expand_the_compact_record away from f0 = 1: mvba_debug_read expands the
    64-byte record on the host (expand_compact_record; the u, v columns are implied).  Against the full-record engine on the same
    pixel problem: residual, J_X and the f, u, v, t columns of J_C bit for bit (K1 stores the same values in either layout), the
    omega columns -- (row of J_X) x (X - t) on the host against K1's own -- within that test's 1e-12 of max|J_C|; and the u, v
    columns are exactly 1 / 600 and 0 where the model says so."""
    shape = FORM["lanes"][1]
    px, _, D = _problem(*shape, 600.0)
    _set_env(monkeypatch, FORM["lanes"][2])
    c = _hip(px)
    _set_env(monkeypatch, FORM["lanes_full"][2])
    f = _hip(px)
    print(f"{shape} f0 = 600: {_assert_form('lanes', 'slots', c)} against {_assert_form('lanes_full', 'slots', f)}")
    c.linearize(), f.linearize()
    np.testing.assert_array_equal(c.debug_read("residual"), f.debug_read("residual"))
    np.testing.assert_array_equal(c.debug_read("JX"), f.debug_read("JX"))
    Jc, Jf = c.debug_read("JC").reshape(-1, 2, 9), f.debug_read("JC").reshape(-1, 2, 9)
    np.testing.assert_array_equal(Jc[:, :, :6], Jf[:, :, :6])
    for J in (Jc, Jf):
        assert (J[:, 0, 1] == 1.0 / 600.0).all() and (J[:, 1, 2] == 1.0 / 600.0).all()
        assert (J[:, 0, 2] == 0.0).all() and (J[:, 1, 1] == 0.0).all()
    assert np.abs(Jf[:, :, 0]).max() > 0
    # (max|J_C| in the twin's units, J_C D, as everywhere in this file: unscaled the pose columns are the largest all the same)
    dev = np.abs(Jc - Jf).max() / np.abs(Jf).max()
    dev_twin = np.abs((Jc - Jf) * D[:9]).max() / np.abs(Jf * D[:9]).max()
    print(f"  J_C compact vs full: max|d| / max|J_C| = {dev:.3e}, column-scaled {dev_twin:.3e} (bound 1e-12)")
    assert np.abs(Jf[:, :, 6:]).max() > 0 and dev <= 1e-12 and dev_twin <= 1e-12


# ---------------------------------------------------------------- covariances
def _cov(eng):
    got = eng.covariance(full=True)
    return {"cov_points": got["points"], "cov_cameras": got["cameras"], "cov_full": got["cameras_full"]}


@pytest.mark.parametrize("name", ["pairs", "dense_full", "gcam", "lanes"])
def test_covariances(monkeypatch, name):
    """The point pass is handed 1 / f0 and the camera blocks come from the inverse of the unscaled S: at 512 the points are
    bitwise the twin's and the camera blocks bitwise the twin's times D_i D_j; at 600 the rule of
    test_every_schur_form_and_the_646_camera_boundary after scaling -- 1e-8 against the reference formulas on the engine's own S,
    1e-7 against schur_covariance.  "lanes": on the compact record mvba_covariance linearises a second time, into a full-layout
    buffer of its own, and its point pass reads that one.  (Its 7e-9 against the 1e-8 is the reference's share: cond(S) = 1.2e11
    on that scene, and np.linalg.inv of the oracle's own S moves by 6.0e-9 of its largest entry under one refinement step in
    extended precision -- DESIGN.md §5.)"""
    _, shape, env, kernel = FORM[name]
    _set_env(monkeypatch, env)
    m = shape[1]
    px, twin, D = _problem(*shape, 512.0)
    a, b = _hip(px), _hip(twin)
    print(f"{name} {shape} covariance f0 = 512, {_assert_form(name, kernel, a, b)}")
    assert_twin(_cov(a), _cov(b), D, exact=True)
    del a, b
    px, _, D = _problem(*shape, 600.0)
    eng = _hip(px)
    _assert_form(name, kernel, eng)
    got = {k: to_twin_units(k, v, D) for k, v in _cov(eng).items()}
    A = eng.debug_read("A_full").reshape(9 * m, 9 * m)
    A = (np.triu(A) + np.triu(A, 1).T) * np.outer(D, D)  # the engine's own undamped S, in the twin's units
    g = make_engine(O.OracleEngine, px)
    g.linearize()
    sig = np.zeros_like(A)
    sig[np.ix_(g.keep, g.keep)] = np.linalg.inv(A[np.ix_(g.keep, g.keep)])
    ref = {"cov_points": point_blocks(g.E, g.F * D[:9], px[2], px[3], sig), "cov_full": 2.0 * sig}
    ref["cov_cameras"] = np.stack([ref["cov_full"][9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(m)])
    ro = schur_covariance(*px)
    ref_o = {k: to_twin_units(k, ro[s], D) for k, s in (("cov_points", "points"), ("cov_cameras", "cameras"), ("cov_full", "cameras_full"))}
    print(f"{name} {shape} covariance f0 = 600")
    for k in ("cov_points", "cov_cameras", "cov_full"):
        _close(got[k], ref[k], 1e-8, k)
        _close(got[k], ref_o[k], 1e-7, k + " (oracle S)")


# ---------------------------------------------------------------- the public path
def test_public_adjuster_in_pixel_units():
    """BundleAdjuster.from_observations(..., f0=600) through optimize() and covariance(scale="residual"): the iteration and
    solve counts of its twin adjuster, K[2, 2] = 600, and f / u variances f0^2 times the twin's (1e-8 of the largest)."""
    px, twin, D = _problem(300, 8, 0.5, 600.0)
    out = []
    for n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R in (px, twin):
        ba = BundleAdjuster.from_observations(n, m, pt_ptr, cam, xy, X, intrinsics_from(f, u, f0), R, t, f0=f0, axis=axis)
        with contextlib.redirect_stdout(io.StringIO()):
            Xo, K, Ro, to = ba.optimize(2.0, 1e-8, 30, is_debug=True)
        cov = ba.covariance(scale="residual")
        out.append((len(ba.get_log()), ba._engine.n_solves, Xo, K, Ro, to, cov))
    (la, sa, Xa, Ka, Ra, ta, ca), (lb, sb, Xb, Kb, Rb, tb, cb) = out
    print(f"public path: {la - 1} iterations / {sa} solves at f0 = 600, {lb - 1} / {sb} on the twin")
    assert la == lb and sa == sb and 2 < la - 1 < 30
    assert (Ka[:, 2, 2] == 600.0).all() and (Kb[:, 2, 2] == 1.0).all()
    _close(Ka[:, :2, :] / 600.0, Kb[:, :2, :], 1e-9, "K / f0")
    _close(Xa, Xb, 1e-9, "X")
    _close(ca["sigma2"], cb["sigma2"], 1e-9, "sigma2")
    va = np.stack([ca["cameras"][:, i, i] for i in range(3)], axis=1)
    vb = np.stack([cb["cameras"][:, i, i] for i in range(3)], axis=1)
    assert (vb > 0).all()
    _close(va / 600.0 ** 2, vb, 1e-8, "var(f, u, v) / f0^2")
    _close(to_twin_units("cov_cameras", ca["cameras"], D), cb["cameras"], 1e-8, "camera blocks")
    _close(ca["points"], cb["points"], 1e-8, "point blocks")
