"""K3's forms and the index builds of mvba_create on IRREGULAR visibility: the structured families of tests/_visibility_cases.py
(banded, hub, two clusters, a few heavy points; tests/test_visibility_cases_cpu.py shows on the host which part of
csrc/mvba_create.h each one reaches) through the comparisons the iid scenes of test_gpu_parity.py, test_gpu_covariance.py and
test_gpu_robust.py go through, at those tests' tolerances.  Every case asserts the form it ran and that the solve stayed on
the Cholesky path."""
import functools

import numpy as np
import pytest

import _visibility_cases as V
from _parity_checks import check_one_step, check_reduced_system
from lib.bundle_adjustment import BundleAdjuster, lm_loop
from test_gpu_parity import slot_index_builds_agree, unit_index_builds_agree

pytestmark = pytest.mark.gpu

C = 1e-2
FORMS = {  # id: (MVBA_SCHUR, MVBA_FORCE_BIG, the form schur_info() must report)
    "slots": ("slots", None, "slots"),
    "pairs": ("pairs", None, "pairs"),     # the unit form's 32-bit-offset build
    "pairs-big": ("pairs", "1", "pairs"),  # ... and its 64-bit-offset build
    "dense": ("dense", None, "dense"),     # through the (point, camera) table: 22 % / 25 % fill
}


def _engine(name, form, monkeypatch):
    schur, big, kernel = FORMS[form]
    monkeypatch.setenv("MVBA_SCHUR", schur)
    if big:
        monkeypatch.setenv("MVBA_FORCE_BIG", big)
    sc, pt_ptr, cam_idx, xy = V.case(name)
    ba = BundleAdjuster.from_observations(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, sc.init_X, sc.init_K, sc.init_R,
                                          sc.init_t, axis=sc.axis)
    assert ba._engine.schur_info()["kernel"] == kernel
    return ba._engine


@functools.lru_cache(maxsize=None)
def _oracle_system(name):
    """(A, b, trial cost) of the oracle at the case's initial state and damping C: computed once, read by every form."""
    g = V.oracle_for(name)
    g.linearize()
    A, b = g.reduced_system(C)
    E1o = g.try_step(C)
    assert np.linalg.eigvalsh(g.A).min() > 0  # positive definite: the engine has no reason to leave the Cholesky path
    A.setflags(write=False), b.setflags(write=False)
    return A, b, E1o


EVERY_FORM = [(name, form) for name in V.TABLE for form in ("slots", "pairs", "pairs-big")] + \
             [("band_3000x14", "dense"), ("blocks_20000x20", "dense")]


@pytest.mark.parametrize("name,form", EVERY_FORM)
def test_every_form_on_every_family_matches_the_oracle(name, form, monkeypatch):
    """The reduced system and the trial cost of one step, per family and form, against the oracle's."""
    eng = _engine(name, form, monkeypatch)
    check_reduced_system(eng, *_oracle_system(name), C)
    assert eng.stats()["counts"]["lu_fallback"] == 0


@pytest.mark.parametrize("form", list(FORMS))
def test_band_every_kernel_output_of_one_step(form, monkeypatch):
    """band 3000 x 14 (point degrees 2 .. 4) through every kernel of a step -- K1's residuals, Jacobians and point sums, the
    point inverse, K3, the solve, K5 / K6's dX and the trial state -- in each form of K3."""
    eng = _engine("band_3000x14", form, monkeypatch)
    g = V.oracle_for("band_3000x14")
    check_one_step(eng, g, C)
    assert eng.stats()["counts"]["lu_fallback"] == 0


def test_skew_idling_lists_that_start_far_apart_inside_one_range(monkeypatch):
    """The bounded-skew merge with slots that idle: a band scene whose slot plan has 8 ranges wider than 2 x SLOT_SKEW
    observations, in which lists sharing a wave begin more than SLOT_SKEW observations apart (asserted from the inputs alone).
    The device-built index must be the host-built one there, hold padding rows, and the kernel on it must give the oracle's
    reduced system."""
    sc, pt_ptr, cam_idx, xy = V.case(V.SKEW_CASE)
    assert V.skew_precondition(pt_ptr, cam_idx, sc.n_images)
    index, info = slot_index_builds_agree(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, sc, monkeypatch)
    _device_took_the_restated_range_plan(V.SKEW_CASE, index)
    assert info["slot_rows"] > info["items"]  # idle slots: padding rows in the step-major index
    monkeypatch.delenv("MVBA_INDEX")
    eng = _engine(V.SKEW_CASE, "slots", monkeypatch)
    check_reduced_system(eng, *_oracle_system(V.SKEW_CASE), C)
    assert eng.stats()["counts"]["lu_fallback"] == 0


def _device_took_the_restated_range_plan(name, index):
    """The pacing table has one row of nSeg entries per wave, and a range plan of nR ranges has slot_waves x nR waves: its size
    shows that mvba_create cut the points into the nR ranges that tests/_visibility_cases.py restates on the host."""
    sc, pt_ptr, cam_idx, _ = V.case(name)
    target, _, slot_waves = V.size_pair_lists(V.pair_counts(pt_ptr, cam_idx, sc.n_images))
    lo = V.slot_ranges(pt_ptr, target, slot_waves)
    n_seg = max(1, int(-(-np.diff(pt_ptr[lo]).max() // V.SLOT_SEG)))
    assert index["index_seg"].size == slot_waves * (len(lo) - 1) * n_seg


INDEX_CASES = ("band_30000x24", "hub_20000x40", "heavy_1500x60", "blocks_20000x20")


@pytest.mark.parametrize("hist", ["lds", "global"])
@pytest.mark.parametrize("name", INDEX_CASES)
def test_slot_index_built_on_the_device_is_the_host_built_one(name, hist, monkeypatch):
    """Empty pairs (slots without a unit among live ones), 256 sub-lists of one pair, point ranges without a point: the
    device's counting sort, dealing and bounded-skew merge against the host threads', entry for entry (index_k / l / a / seg
    and schur_info()), with the wave's pair histogram in LDS and in device memory."""
    sc, pt_ptr, cam_idx, xy = V.case(name)
    index, _ = slot_index_builds_agree(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, sc, monkeypatch, hist)
    _device_took_the_restated_range_plan(name, index)


@pytest.mark.parametrize("hist", ["lds", "global"])
@pytest.mark.parametrize("name", INDEX_CASES)
def test_unit_index_built_on_the_device_is_the_host_built_one(name, hist, monkeypatch):
    """The unit form's index on the same scenes (units skipped where a list has no item in a range, queues of unequal
    length): entry for entry, and A_full and dxi of one trial bit for bit."""
    sc, pt_ptr, cam_idx, xy = V.case(name)
    unit_index_builds_agree(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, sc, monkeypatch, hist)


@functools.lru_cache(maxsize=None)
def _oracle_short_run(name):
    g = V.oracle_for(name)
    g.n_solves = 0
    return lm_loop(g, 2.0, -1.0, 5, verbose=False), g.n_solves


@pytest.mark.parametrize("form", ["slots", "pairs"])
@pytest.mark.parametrize("name", ["hub_20000x40", "band_3000x14"])
def test_short_lm_run_matches_the_oracle(name, form, monkeypatch):
    """Five outer LM iterations as in test_random_scene_one_step_and_short_run_vs_oracle: the same accept / reject sequence
    and the same final RMSE to 1e-9."""
    eng = _engine(name, form, monkeypatch)
    n_obs = len(V.case(name)[2])
    eng.n_solves = 0
    Eg = lm_loop(eng, 2.0, -1.0, 5, verbose=False)
    Eo, n_solves = _oracle_short_run(name)
    assert eng.n_solves == n_solves
    assert abs(np.sqrt(Eg / n_obs) - np.sqrt(Eo / n_obs)) < 1e-9
    assert eng.stats()["counts"]["lu_fallback"] == 0


def _band_problem(xy=None):
    from lib.bundle_adjustment import to_gauge_frame

    sc, pt_ptr, cam_idx, xy0 = V.case("band_3000x14")
    X, R, t = to_gauge_frame(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    return (sc.n_points, sc.n_images, pt_ptr, cam_idx, xy0 if xy is None else xy, 1.0, sc.axis, X, sc.init_K[:, 0, 0],
            sc.init_K[:, :2, 2], t, R)


def test_band_covariance_matches_the_reference():
    """Marginal covariances at point degrees 2 .. 4 against tests/_covariance_ref.py, at test_random_scenes_match_the_reference's
    tolerance."""
    from test_gpu_covariance import _check

    m = 14
    got = _check(_band_problem())
    assert np.array_equal(got["cameras"], np.stack([got["cameras_full"][9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(m)]))


def test_band_huber_step_matches_the_reference():
    """A Huber engine (the robust unit form) on band with gross outliers, against tests/_robust_ref.py, at
    test_reduced_system_and_step_match_the_reference's tolerances."""
    from _robust_ref import inject_outliers
    from test_gpu_robust import _check_step, _engines

    xy, _ = inject_outliers(np.array(V.case("band_3000x14")[3]), 0.08, 20.0, 100.0, seed=5)
    eng, g = _engines(_band_problem(xy), "huber", 3.0)
    assert eng.schur_info()["kernel"] == "pairs"
    _check_step(eng, g)
    assert g.w.min() < 0.5  # the outliers are down-weighted
    assert eng.stats()["counts"]["lu_fallback"] == 0


def test_hub_two_engines_are_bitwise_identical():
    """Two engines on hub (the form mvba_create takes by itself: the unit form, 256 sub-lists on one pair): A_full and dxi bit
    for bit."""
    sc, pt_ptr, cam_idx, xy = V.case("hub_20000x40")
    out = []
    for _ in range(2):
        eng = BundleAdjuster.from_observations(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, sc.init_X, sc.init_K, sc.init_R,
                                               sc.init_t, axis=sc.axis)._engine
        assert eng.schur_info()["kernel"] == "pairs"
        eng.linearize()
        E1 = eng.try_step(C)
        out.append((E1, eng.debug_read("A_full").copy(), eng.debug_read("dxi").copy()))
        assert eng.stats()["counts"]["lu_fallback"] == 0
    assert out[0][0] == out[1][0]
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][2], out[1][2])
