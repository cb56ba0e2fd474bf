"""The code the engine picks by a point's degree, on the families of tests/_degree_cases.py (tests/test_degree_cases_cpu.py
shows on the host which tile layout, K5 cell and covariance width each one reaches), through the shared comparisons of
tests/_parity_checks.py, test_gpu_covariance.py, test_gpu_robust.py, test_gpu_parity.py and test_gpu_point_hold.py at those
tests' tolerances.

What each test is the first to run:
  test_one_step_every_kernel_output     k_resid_jac's split branch beside packed tiles, ~0 first, the terminator after a split
                                        tile, 3 .. 5 pieces, a last piece of one; tile_slot with -1 between slots; k_sum_split
                                        over unequal piece counts (E, dP); k_backsub<8, 256 | 512 | 1024 | GCAM>,
                                        k_backsub<4, 512 | 1024 | GCAM> (dX, trial_X); k_backsub<2> on degree 64 .. 300 (its
                                        one-by-one loop beyond four observations per lane for 32 .. 150 trips)
  test_every_k3_form_on_a_cut_point     k_schur_slots, k_schur_lanes and both builds of k_schur_pairs reading the records and
                                        the point inverse of a point cut into pieces
  test_*_index_built_on_the_device...   k_idx_count / k_idx_fill's row loop beyond two trips (rows of 65 .. 300), with the
                                        histogram in LDS and in device memory (300 cameras: device memory by itself)
  test_robust_twins                     robust k_resid_jac on split tiles; the robust k_backsub<G, bt, GCAM, true> at every
                                        (G, bt) but (2, 256) and (2, GCAM) (the prefetch of sqw on clamped indices at widths
                                        2, 4 and 8; the table below has the case of each cell)
  test_covariance                       k_point_cov<8> on points of 3 240 / 8 515 pairs (the sqrt pair decode far from the
                                        pair counts it is sized for), k_point_cov<64> at degree 110
  test_held_points_on_split_tiles       k_point_inv with a mask over points whose sums come from k_sum_split
  test_engine_triangulation_...         k_triangulate's per-point loops at degree 300 inside the engine
  test_two_engines_... / test_short_... run-to-run identity and five LM iterations of all of the above

Every robust (G, bt) cell of k_backsub is run, by the case of test_robust_twins named here (the last four are the iid scenes
of _degree_cases.ROBUST_WIDE, which only the robust twins use) or by tests/test_gpu_robust.py:
  bt        G = 2                         G = 4                 G = 8
  256       tests/test_gpu_robust.py      wide_60x90_60         wide_40x110
            (and tall_2000x130)
  512       wide_300x200_10               wide_60x200_35        wide_60x200_60
  1024      wide_300x400_05               wide_120x400_15       wide_60x400_35
  GCAM      tests/test_gpu_robust.py      wide_200x647_10       wide_80x647_20"""
import functools

import numpy as np
import pytest

import _degree_cases as D
from _parity_checks import check_one_step, check_reduced_system
from lib.bundle_adjustment import BundleAdjuster, lm_loop, parameter_map
from test_gpu_parity import slot_index_builds_agree, unit_index_builds_agree

pytestmark = pytest.mark.gpu

C = 1e-2


def _engine(name, monkeypatch=None, schur=None, big=None, init_X=True):
    if schur:
        monkeypatch.setenv("MVBA_SCHUR", schur)
    if big:
        monkeypatch.setenv("MVBA_FORCE_BIG", big)
    sc, pt_ptr, cam_idx, xy = D.case(name)
    return BundleAdjuster.from_observations(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, sc.init_X if init_X else None,
                                            sc.init_K, sc.init_R, sc.init_t, axis=sc.axis)._engine


@functools.lru_cache(maxsize=None)
def _oracle_system(name):
    """(A, b, trial cost) of the shared oracle at the case's initial state and damping C."""
    g = D.oracle_for(name)
    g.linearize()
    A, b = g.reduced_system(C)
    E1o = g.try_step(C)
    np.linalg.cholesky(g.A)  # positive definite: the engine has no reason to leave the Cholesky path
    return A, b, E1o


# ---------------------------------------------------------------- 1: one whole step
@pytest.mark.parametrize("name", D.CASES)
def test_one_step_every_kernel_output(name):
    """Residuals, JX, JC, E, dP (the split path and k_sum_split), A_full, b_full, dxi, dX and the trial state (K5) against the
    oracle, in the form of K3 the engine picks by itself."""
    eng = _engine(name)
    check_one_step(eng, D.oracle_for(name), C)
    assert eng.stats()["counts"]["lu_fallback"] == 0


# ---------------------------------------------------------------- 2: every K3 form on a cut point
K3_FORMS = {  # id: (MVBA_SCHUR, MVBA_FORCE_BIG, kernel, step_width)
    "slots": ("slots", None, "slots", 21),
    "lanes": ("lanes", None, "slots", 64),
    "pairs": ("pairs", None, "pairs", 0),
    "pairs-big": ("pairs", "1", "pairs", 0),
}
K3_RUNS = [("tall_1500x80", f) for f in K3_FORMS] + [(n, f) for n in ("tall_2000x130", "tall_6000x300") for f in ("pairs", "pairs-big")]


@pytest.mark.parametrize("name,form", K3_RUNS)
def test_every_k3_form_on_a_cut_point(name, form, monkeypatch):
    schur, big, kernel, width = K3_FORMS[form]
    eng = _engine(name, monkeypatch, schur, big)
    info = eng.schur_info()
    assert info["kernel"] == kernel and info["step_width"] == width, info
    check_reduced_system(eng, *_oracle_system(name), C)
    assert eng.stats()["counts"]["lu_fallback"] == 0


# ---------------------------------------------------------------- 3: the index builds
@pytest.mark.parametrize("hist", ["lds", "global"])
def test_slot_index_built_on_the_device_is_the_host_built_one(hist, monkeypatch):
    sc, pt_ptr, cam_idx, xy = D.case("tall_1500x80")
    slot_index_builds_agree(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, sc, monkeypatch, hist)


@pytest.mark.parametrize("hist", ["lds", "global"])
@pytest.mark.parametrize("name", list(D.TALL))
def test_unit_index_built_on_the_device_is_the_host_built_one(name, hist, monkeypatch):
    """The device's walk of rows longer than 64, 128 and 256 against the host's, entry for entry, and one trial bit for bit."""
    sc, pt_ptr, cam_idx, xy = D.case(name)
    unit_index_builds_agree(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, sc, monkeypatch, hist)


# ---------------------------------------------------------------- 4: the robust twins
@pytest.mark.parametrize("loss,scale", D.ROBUST_LOSSES)
@pytest.mark.parametrize("name", D.ROBUST_CASES)
def test_robust_twins(name, loss, scale):
    """tests/test_gpu_robust.py::_check_step at its bounds, at damping ROBUST_C = 1e-2: at that helper's default 1e-3 the first
    Huber trial on wide_80x647_20 is a camera update of 139 whose cost the reference itself fixes to 7.2e-10 only (the device
    came within 3.9e-9 of it there, every other output within its bound); tests/_degree_cases.py has the figures, and
    tests/test_degree_cases_cpu.py holds the reference to 1e-11 at 1e-2 for every twin."""
    from test_gpu_robust import _check_step, _engines

    eng, g = _engines(D.problem(name, D.outlier_xy(name)), loss, scale)
    assert eng.schur_info()["kernel"] == "pairs"
    _check_step(eng, g, c=D.ROBUST_C)
    assert g.w.min() < 0.5  # the outliers are down-weighted


# ---------------------------------------------------------------- 5: covariance
@pytest.mark.parametrize("name", ["tall_1500x80", "tall_2000x130", "wide_40x110"])
def test_covariance(name):
    from test_gpu_covariance import _check, _engine as cov_engine

    prob = D.problem(name)
    _check(prob)
    eng = cov_engine(prob)
    a, b = eng.covariance(full=True), eng.covariance(full=True)
    for k in ("points", "cameras", "cameras_full"):
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 6: held points
def test_held_points_on_split_tiles():
    """tall_2000x130 with the split points 8 and 1000 held, the split points 0, 9 and 1999 free, and every third short point
    held: one step at two dampings against tests/_point_hold_ref.py, bounds and exact checks of
    tests/test_gpu_point_hold.py::test_one_step_for_every_kind_of_mask."""
    from test_gpu_point_hold import _check_held_step, _hold, _pair

    n, m, pt_ptr, cam, xy, _, axis, *state = D.problem("tall_2000x130")
    tall = D.TALL["tall_2000x130"][2]
    mask = np.arange(n) % 3 == 2
    mask[list(tall)] = False
    mask[[8, 1000]] = True
    assert not mask[[0, 9, 1999]].any() and mask.sum() > n // 4
    eng, ref = _pair(n, m, pt_ptr, cam, xy, axis, tuple(state))
    eng.linearize()
    ref.linearize()
    E6, dP = eng.debug_read("E"), eng.debug_read("dP")
    col, n_free = parameter_map(m, axis)
    _hold(eng, ref, mask, col, n_free)
    for c in (1e-4, 1e-1):
        _check_held_step(eng, ref, mask, col, n_free, c, state[0])
    assert np.array_equal(eng.debug_read("E"), E6) and np.array_equal(eng.debug_read("dP"), dP)
    dX = eng.debug_read("dX").reshape(-1, 3)
    assert (dX[[0, 9, 1999]] != 0).all()
    assert eng.stats()["counts"]["lu_fallback"] == 0


# ---------------------------------------------------------------- 7: engine-resident triangulation
def test_engine_triangulation_of_degree_300_points():
    """init_X=None on tall_6000x300 against tests/_init_ref.py, at MARGIN x the host-versus-host figure of this very case."""
    from test_gpu_init import _close

    eng = _engine("tall_6000x300", init_X=False)
    Xr, _, sr = D.tri_reference("tall_6000x300")
    assert (sr == 0).all()
    _close(eng.get_params()[0], Xr, D.MARGIN * D.TRI_HOST_DIFF, "tall_6000x300 init_X=None")


# ---------------------------------------------------------------- 8: determinism and a short run
@pytest.mark.parametrize("name", ["tall_2000x130", "wide_60x400_35"])
def test_two_engines_are_bitwise_identical(name):
    out = []
    for _ in range(2):
        eng = _engine(name)
        eng.linearize()
        E1 = eng.try_step(C)
        out.append((E1, eng.debug_read("A_full").copy(), eng.debug_read("dxi").copy(), eng.debug_read("dX").copy()))
        assert eng.stats()["counts"]["lu_fallback"] == 0
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        np.testing.assert_array_equal(a, b)


@functools.lru_cache(maxsize=None)
def _oracle_short_run(name):
    from oracle import ba_oracle as O

    sc, pt_ptr, cam_idx, xy = D.case(name)
    g = O.OracleEngine(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, 1.0, sc.axis)  # (its own: this one is committed)
    g.set_params(*D.oracle_for(name).get_params())
    return lm_loop(g, 2.0, -1.0, 5, verbose=False), g.n_solves


@pytest.mark.parametrize("name", ["tall_1500x80", "wide_40x110"])
def test_short_lm_run_matches_the_oracle(name):
    """Five outer LM iterations as tests/test_gpu_visibility.py::test_short_lm_run_matches_the_oracle: the same accept / reject
    sequence, the same solve count, the final RMSE to 1e-9."""
    eng = _engine(name)
    n_obs = len(D.case(name)[2])
    eng.n_solves = 0
    Eg = lm_loop(eng, 2.0, -1.0, 5, verbose=False)
    Eo, n_solves = _oracle_short_run(name)
    assert eng.n_solves == n_solves
    assert abs(np.sqrt(Eg / n_obs) - np.sqrt(Eo / n_obs)) < 1e-9
    assert eng.stats()["counts"]["lu_fallback"] == 0
