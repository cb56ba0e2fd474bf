"""The lane form (k_schur_lanes, k_schur_lanes_compact; MVBA_SCHUR=lanes) on the packed 512-byte index row with its point ranges
counted by wave places: any number of ranges from 1 on, forced with MVBA_SLOT_RANGES -- below 8, no multiple of 8, and 11 ranges
of 96 waves, more waves than the chip has places (the launch is not paced: the surplus runs later).  Against the oracle, device-
against host-built index, two engines, compact against full record, offsets l - k past 64, and what schur_info() reports of the
plan: the ranges and the waves per CU the occupancy query answered (four for the compact kernel; three would be a silent
fall-back to the plan before the packed row).

Bounds: tests/_parity_checks.py::check_reduced_system (A 1e-11 max|A|, b 1e-9 max|b|) as tests/test_gpu_schur_lanes.py; compact
against full 2e-11 / 2e-9 as tests/test_gpu_compact_record.py.  The number of ranges changes how many partials a pair's block
is summed from, not the bounds."""
import numpy as np
import pytest

import _visibility_cases as V
from _parity_checks import check_reduced_system
from test_gpu_compact_record import _engine as _record_engine, _env, _same_step, _scene, _trial
from test_gpu_schur_lanes import _case_system, _oracle, _oracle_system
from test_lanes_ranges_cpu import CUS, lane_ranges, lane_waves, wide_case

pytestmark = pytest.mark.gpu

C = 1e-2
PLACES = {"compact": 4, "full": 3}  # waves per CU: 40,960 B (four in 160 KiB) and 53,248 B of LDS


def _engine(sc, n_ranges, record="compact", obs=None, **env):
    """A lane-form engine at `n_ranges` forced ranges (None: mvba_create's own count); asserts the plan schur_info() reports."""
    with _env(**({"MVBA_SLOT_RANGES": str(n_ranges)} if n_ranges else {}), **env):
        eng = _record_engine(sc, record, obs)
    info = eng.schur_info()
    assert info["places_per_cu"] == PLACES[record], info
    assert n_ranges is None or info["ranges"] == n_ranges, info
    return eng


_SYSTEMS = {}


def _scene_system(shape):
    if shape not in _SYSTEMS:
        A, b, E1 = _oracle_system(_oracle(_scene(*shape)))
        A.setflags(write=False), b.setflags(write=False)
        _SYSTEMS[shape] = (A, b, E1)
    return _SYSTEMS[shape]


@pytest.mark.parametrize("n_ranges", [1, 3, 10, 11])
@pytest.mark.parametrize("shape", [(2000, 100, 0.1), (3000, 30, 0.3)])
def test_one_trial_matches_the_oracle(shape, n_ranges):
    """96 waves per range (the capacity edge; at 11 ranges 1056 waves on 1024 places) and 9."""
    eng = _engine(_scene(*shape), n_ranges)
    check_reduced_system(eng, *_scene_system(shape), C)
    assert eng.stats()["counts"]["lu_fallback"] == 0


def test_an_empty_point_range_at_ten_ranges():
    """heavy_1500x60: points that carry more items than a range's share -- ranges without a point, waves without a step."""
    sc, pt_ptr, cam_idx, xy = V.case("heavy_1500x60")
    eng = _engine(sc, 10, obs=(pt_ptr, cam_idx, xy))
    check_reduced_system(eng, *_case_system("heavy_1500x60"), C)
    assert eng.stats()["counts"]["lu_fallback"] == 0


def test_index_built_on_the_device_is_the_host_built_one():
    """4000 x 100 x 0.1 at 10 ranges: the unpacked index rows entry for entry, one trial bit for bit."""
    sc = _scene(4000, 100, 0.1)
    dev, host = _engine(sc, 10), _engine(sc, 10, MVBA_INDEX="host")
    assert dev.schur_info() == host.schur_info()
    for k in ("index_k", "index_l", "index_a"):
        d = dev.debug_read(k)
        assert d.size == dev.schur_info()["slot_rows"] > 0
        np.testing.assert_array_equal(d, host.debug_read(k), err_msg=k)
    a, b = _trial(dev), _trial(host)
    for k in ("A", "b", "dxi", "tX"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_two_engines_are_bitwise_identical():
    """One partial per list and range, summed in list order: no multiple of 8 changes that."""
    sc = _scene(3000, 30, 0.3)
    a, b = _trial(_engine(sc, 10)), _trial(_engine(sc, 10))
    for k in ("A", "b", "dxi", "tX"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("n_ranges", [3, 10])
def test_compact_matches_the_full_record(n_ranges):
    """Four waves per CU against three, the same ranges and the same packed rows."""
    sc = _scene(2000, 100, 0.1)
    _same_step(_trial(_engine(sc, n_ranges)), _trial(_engine(sc, n_ranges, "full")))


def test_offsets_past_64():
    """tests/test_gpu_compact_record.py::_wide_case, points seen by all 80 cameras: l - k up to 79 in the index rows as the
    kernel reads them, and the reduced system against the oracle at 10 ranges.  (Why no scene here reaches the offset's high
    field: tests/test_lanes_ranges_cpu.py::test_the_wide_case_reaches_offsets_past_64.)"""
    sc, obs = wide_case()
    eng = _engine(sc, 10, obs=obs)
    k, l, a = (eng.debug_read(x).astype(np.int64) for x in ("index_k", "index_l", "index_a"))
    real = a < sc.n_points  # (the padding rows: record 0 twice, point row N)
    assert (l - k).max() == 79 and (l >= k).all() and (k[~real] == 0).all() and (l[~real] == 0).all()
    o0 = np.asarray(obs[0])
    assert ((l - k)[real] < (o0[1:] - o0[:-1])[a[real]]).all()  # below the degree of the item's point
    got = _trial(eng)
    A, b, E1o = _oracle_system(_oracle(sc, *obs))
    np.testing.assert_allclose(got["A"], A, rtol=0, atol=1e-11 * np.abs(A).max())
    np.testing.assert_allclose(got["b"], b, rtol=0, atol=1e-9 * np.abs(b).max())
    assert got["E1"] == pytest.approx(E1o, rel=1e-7)


def test_the_plan_mvba_create_makes_by_itself():
    """Small scenes are capped at 8 ranges; 110,000 x 100 x 10 % (a typical list of 1024 items or more) takes the count of the
    places: 10 ranges on four waves per CU (tests/test_lanes_ranges_cpu.py restates the rule), and one trial is finite."""
    sc = _scene(2000, 100, 0.1)
    assert _engine(sc, None).schur_info()["ranges"] == 8 == _engine(sc, None, "full").schur_info()["ranges"]
    big = _scene(110000, 100, 0.1)
    waves, target = lane_waves(big.pt_ptr, big.cam_idx, 100)
    eng = _engine(big, None)
    info = eng.schur_info()
    assert info["ranges"] == lane_ranges(PLACES["compact"] * CUS, waves, target) == 10, info
    eng.linearize()
    assert np.isfinite(eng.try_step(C)) and eng.stats()["counts"]["lu_fallback"] == 0
