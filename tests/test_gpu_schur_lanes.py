"""K3's slot form with one lane per item (k_schur_lanes: 64 lists per wave, csrc/mvba_lanes.h), forced with MVBA_SCHUR=lanes:
against the oracle and against k_schur_slots on the same scenes, its fallback where a point range needs more than 96 waves,
irregular visibility, the index build at width 64 on the device and on host threads, reproducibility, and the selection
mvba_create makes by itself.  schur_info() reports the form as "slots" with step_width 64 (21: k_schur_slots)."""
import functools

import numpy as np
import pytest

import _visibility_cases as V
from _parity_checks import check_reduced_system
from lib.bundle_adjustment import BundleAdjuster, lm_loop
from lib.synthetic import make_scene
from oracle import ba_oracle as O

pytestmark = pytest.mark.gpu

C = 1e-2


@functools.lru_cache(maxsize=None)
def _scene(n, m, p):
    return make_scene(n, m, vis_p=p)


def _engine(sc, pt_ptr=None, cam_idx=None, xy=None):
    pt_ptr, cam_idx, xy = (sc.pt_ptr, sc.cam_idx, sc.xy) if pt_ptr is None else (pt_ptr, cam_idx, xy)
    return BundleAdjuster.from_observations(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, sc.init_X, sc.init_K, sc.init_R,
                                            sc.init_t, axis=sc.axis)._engine


def _oracle(sc, pt_ptr=None, cam_idx=None, xy=None):
    pt_ptr, cam_idx, xy = (sc.pt_ptr, sc.cam_idx, sc.xy) if pt_ptr is None else (pt_ptr, cam_idx, xy)
    g = O.OracleEngine(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, 1.0, sc.axis)
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    g.set_params(X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)
    return g


def _oracle_system(g):
    g.linearize()
    A, b = g.reduced_system(C)
    return A, b, g.try_step(C)


def _took(eng, width):
    info = eng.schur_info()
    assert info["kernel"] == "slots" and info["step_width"] == width, info
    return info


def _system(eng):
    eng.linearize()
    eng.try_step(C)
    m9 = 9 * eng.m
    return eng.debug_read("A_full").reshape(m9, m9), eng.debug_read("b_full")


def _lane_waves(pt_ptr, cam_idx, m):
    """Waves of 64 lists a point range needs (csrc/mvba_create.h, PairLists::slot_waves, restated)."""
    _, S, _ = V.size_pair_lists(V.pair_counts(pt_ptr, cam_idx, m))
    return -(-int(np.trace(S)) // 64) + -(-int(S[np.triu_indices(m, 1)].sum()) // 64)


@pytest.mark.parametrize("n,m,p,waves", [(3000, 12, 0.5, 3), (3000, 30, 0.3, 9), (2000, 100, 0.1, 96)])
def test_one_trial_matches_the_oracle_and_the_slot_kernel(n, m, p, waves, monkeypatch):
    """The reduced system and the trial cost of one step at the tolerance of test_every_schur_kernel_form_matches_the_oracle
    (A to 1e-11 max|A|, b to 1e-9 max|b|), and against k_schur_slots on the same scene where that kernel fits -- both sum the
    same items in other orders: twice the bound each has against the oracle.  12 cameras: one diagonal wave and two
    off-diagonal ones, the second with 2 of its 64 lists; 100 cameras: all 96 waves an XCD holds (k_schur_slots' 289 do not
    fit its 288 there)."""
    sc = _scene(n, m, p)
    assert _lane_waves(sc.pt_ptr, sc.cam_idx, m) == waves
    monkeypatch.setenv("MVBA_SCHUR", "lanes")
    eng = _engine(sc)
    info = _took(eng, 64)
    assert info["slot_rows"] % 64 == 0 and info["slot_rows"] >= info["items"]
    check_reduced_system(eng, *_oracle_system(_oracle(sc)), C)
    assert eng.stats()["counts"]["lu_fallback"] == 0
    A, b = _system(eng)
    monkeypatch.setenv("MVBA_SCHUR", "slots")
    ref = _engine(sc)
    if ref.schur_info()["kernel"] != "slots":
        assert m == 100  # (one wave over k_schur_slots' capacity: the unit form stands in, at the same bounds)
    else:
        _took(ref, 21)
    A0, b0 = _system(ref)
    np.testing.assert_allclose(A, A0, rtol=0, atol=2e-11 * np.abs(A0).max())
    np.testing.assert_allclose(b, b0, rtol=0, atol=2e-9 * np.abs(b0).max())


def test_falls_back_at_101_cameras(monkeypatch):
    """2000 x 101 x 0.1 needs 97 waves of 64 lists per range, one more than an XCD holds: MVBA_SCHUR=lanes falls back to
    k_schur_slots, whose 294 waves of 21 do not fit either, and on to the unit form -- the engine mvba_create builds by itself
    there, bit for bit."""
    sc = _scene(2000, 101, 0.1)
    assert _lane_waves(sc.pt_ptr, sc.cam_idx, 101) == 97
    default = _engine(sc)
    monkeypatch.setenv("MVBA_SCHUR", "lanes")
    eng = _engine(sc)
    info = eng.schur_info()
    assert info == default.schur_info() and info["kernel"] == "pairs" and info["step_width"] == 0
    A, b = _system(eng)
    A0, b0 = _system(default)
    np.testing.assert_array_equal(A, A0)
    np.testing.assert_array_equal(b, b0)


@functools.lru_cache(maxsize=None)
def _case_system(name):
    A, b, E1o = _oracle_system(V.oracle_for(name))
    A.setflags(write=False), b.setflags(write=False)
    return A, b, E1o


@pytest.mark.parametrize("name", V.TABLE)
def test_irregular_visibility_matches_the_oracle(name, monkeypatch):
    """The families of tests/_visibility_cases.py: camera pairs without a common point (band, blocks, heavy: lanes without a
    unit among live ones), point ranges without a point (heavy), 256 sub-lists of one pair beside lists of a few items (hub), a
    camera seen by the n_full / bridge points only beside its neighbours."""
    sc, pt_ptr, cam_idx, xy = V.case(name)
    monkeypatch.setenv("MVBA_SCHUR", "lanes")
    eng = _engine(sc, pt_ptr, cam_idx, xy)
    _took(eng, 64)
    check_reduced_system(eng, *_case_system(name), C)
    assert eng.stats()["counts"]["lu_fallback"] == 0


def test_a_camera_with_one_observation(monkeypatch):
    """3000 x 12, every (point, camera) pair kept with probability 0.5 (two views at least), camera 11 seen by point 0 alone: a
    diagonal list of one item, off-diagonal lists of at most one, the others empty."""
    n, m = 3000, 12
    sc = make_scene(n, m, vis_p=1.0, project="numpy")
    keep = np.random.default_rng(V.SEED).random((n, m)) < 0.5
    keep[:, 11] = False
    keep[0, 11] = True
    keep[keep.sum(1) < 2, :2] = True
    pt_ptr, cam_idx, xy = V.masked(sc, keep)
    assert (cam_idx == 11).sum() == 1 and np.diff(pt_ptr).min() >= 2
    monkeypatch.setenv("MVBA_SCHUR", "lanes")
    eng = _engine(sc, pt_ptr, cam_idx, xy)
    _took(eng, 64)
    check_reduced_system(eng, *_oracle_system(_oracle(sc, pt_ptr, cam_idx, xy)), C)


def test_index_built_on_the_device_is_the_host_built_one(monkeypatch):
    """The step-major index at width 64 (4000 x 100 x 0.1: 94 waves per range, padding rows from the bounded-skew merge) from
    the k_idx_* kernels and from MVBA_INDEX=host: index_k / l / a / seg and schur_info() entry for entry, one trial bit for bit."""
    sc = _scene(4000, 100, 0.1)
    monkeypatch.setenv("MVBA_SCHUR", "lanes")
    out = []
    for where in (None, "host"):
        if where:
            monkeypatch.setenv("MVBA_INDEX", where)
        eng = _engine(sc)
        info = _took(eng, 64)
        index = {k: eng.debug_read(k) for k in ("index_k", "index_l", "index_a", "index_seg")}
        out.append((index, info) + _system(eng))
    (dev, info_d, A_d, b_d), (host, info_h, A_h, b_h) = out
    assert info_d == info_h and info_d["slot_rows"] > info_d["items"]
    for k in dev:
        assert dev[k].size > 0
        np.testing.assert_array_equal(dev[k], host[k], err_msg=k)
    np.testing.assert_array_equal(A_d, A_h)
    np.testing.assert_array_equal(b_d, b_h)


def test_two_engines_are_bitwise_identical(monkeypatch):
    """One partial per list, summed in list order by k_schur_reduce: A_full and b_full of two engines on one scene, bit for bit."""
    sc = _scene(3000, 30, 0.3)
    monkeypatch.setenv("MVBA_SCHUR", "lanes")
    (A0, b0), (A1, b1) = (_system(e) for e in (_engine(sc), _engine(sc)))
    np.testing.assert_array_equal(A0, A1)
    np.testing.assert_array_equal(b0, b1)


def test_default_selection_short_run_matches_the_oracle():
    """2000 x 100 x 0.1 in the form mvba_create takes by itself: five outer LM iterations as in
    test_short_lm_run_matches_the_oracle -- the same accept / reject sequence and the same final RMSE to 1e-9."""
    sc = _scene(2000, 100, 0.1)
    eng, g = _engine(sc), _oracle(sc)
    eng.n_solves = g.n_solves = 0
    Eg = lm_loop(eng, 2.0, -1.0, 5, verbose=False)
    Eo = lm_loop(g, 2.0, -1.0, 5, verbose=False)
    assert eng.n_solves == g.n_solves
    assert abs(np.sqrt(Eg / sc.n_obs) - np.sqrt(Eo / sc.n_obs)) < 1e-9
    assert eng.stats()["counts"]["lu_fallback"] == 0
