"""The compact 64-byte linearisation record of the lane-form engines (k_resid_jac<.., CompactRec>,
k_schur_lanes_compact): against the oracle, against the same engine on the full record (MVBA_REC=full), and through the other
readers of the record -- debug reads, covariances, held points, parameter maps, snapshots, two sharded ranks.  Every engine here is forced into
the lane form (MVBA_SCHUR=lanes) and asserts which record it runs on: schur_info()["record"].

Tolerances.  Against the oracle: tests/_parity_checks.py::check_reduced_system (A 1e-11 max|A|, b 1e-9 max|b|, trial cost 1e-7),
what tests/test_gpu_schur_lanes.py holds k_schur_lanes to.  Compact against full: both sum the same items in the same order and
differ in the rounding of J_omega alone; each is within the oracle bound, so twice that between them, as that file compares
k_schur_lanes with k_schur_slots (A 2e-11, b 2e-9).  dxi and the trial points: check_one_step holds an engine to 1e-9 max|dxi|
and 1e-10 (absolute, a normalised scene) against the oracle -- 2e-9 and 2e-10 between two engines."""
import contextlib
import functools
import os

import numpy as np
import pytest

import _visibility_cases as V
from _parity_checks import check_reduced_system
from lib.bundle_adjustment import BundleAdjuster, parameter_map
from lib.synthetic import make_scene
from test_gpu_schur_lanes import _case_system, _oracle, _oracle_system

pytestmark = pytest.mark.gpu

C = 1e-2
SHAPES = [(2000, 100, 0.1), (3000, 30, 0.3), (3000, 12, 0.5)]  # 96 waves per range (the capacity edge), 9, 3


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _scene(n, m, p):
    return make_scene(n, m, vis_p=p)


def _engine(sc, record, obs=None):
    """A lane-form engine on `record` ("compact": what mvba_create takes there; "full": MVBA_REC=full), which it asserts."""
    pt_ptr, cam_idx, xy = (sc.pt_ptr, sc.cam_idx, sc.xy) if obs is None else obs
    with _env(MVBA_SCHUR="lanes", **({"MVBA_REC": "full"} if record == "full" else {})):
        eng = BundleAdjuster.from_observations(sc.n_points, sc.n_images, pt_ptr, cam_idx, xy, sc.init_X, sc.init_K, sc.init_R,
                                               sc.init_t, axis=sc.axis)._engine
    info = eng.schur_info()
    assert info["kernel"] == "slots" and info["step_width"] == 64 and info["record"] == record, info
    return eng


def _trial(eng):
    """One linearisation and one trial: what the step computed."""
    eng.linearize()
    E1 = eng.try_step(C)
    m9 = 9 * eng.m
    return {"A": eng.debug_read("A_full").reshape(m9, m9), "b": eng.debug_read("b_full"), "dxi": eng.debug_read("dxi"),
            "dX": eng.debug_read("dX").reshape(-1, 3), "tX": eng.debug_read("trial_X").reshape(-1, 3), "E1": E1}


def _same_step(got, ref):
    """Compact against full at the bounds of the module docstring; prints each figure first."""
    dev = {k: np.abs(got[k] - ref[k]).max() for k in ("A", "b", "dxi", "tX")}
    print(f"compact vs full: |dA| / max|A| = {dev['A'] / np.abs(ref['A']).max():.3e} (2e-11), |db| / max|b| = "
          f"{dev['b'] / np.abs(ref['b']).max():.3e} (2e-9), |ddxi| / max|dxi| = {dev['dxi'] / np.abs(ref['dxi']).max():.3e} (2e-9), "
          f"|dtX| = {dev['tX']:.3e} (2e-10), trial cost rel. {abs(got['E1'] - ref['E1']) / ref['E1']:.3e} (1e-9)")
    np.testing.assert_allclose(got["A"], ref["A"], rtol=0, atol=2e-11 * np.abs(ref["A"]).max())
    np.testing.assert_allclose(got["b"], ref["b"], rtol=0, atol=2e-9 * np.abs(ref["b"]).max())
    np.testing.assert_allclose(got["dxi"], ref["dxi"], rtol=0, atol=2e-9 * np.abs(ref["dxi"]).max())
    np.testing.assert_allclose(got["tX"], ref["tX"], rtol=0, atol=2e-10)
    assert got["E1"] == pytest.approx(ref["E1"], rel=1e-9)


@functools.lru_cache(maxsize=None)
def _full_trial(n, m, p):
    t = _trial(_engine(_scene(n, m, p), "full"))
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


@pytest.mark.parametrize("n,m,p", SHAPES)
def test_one_trial_matches_the_oracle(n, m, p):
    sc = _scene(n, m, p)
    eng = _engine(sc, "compact")
    check_reduced_system(eng, *_oracle_system(_oracle(sc)), C)
    assert eng.stats()["counts"]["lu_fallback"] == 0


@pytest.mark.parametrize("name", V.TABLE)
def test_irregular_visibility_matches_the_oracle(name):
    """The families of tests/_visibility_cases.py, all of which fit the lane form: lanes without a list among live ones (their
    centre is the zero vector, their rows the padding record), empty point ranges, 256 sub-lists of one pair."""
    sc, pt_ptr, cam_idx, xy = V.case(name)
    eng = _engine(sc, "compact", (pt_ptr, cam_idx, xy))
    check_reduced_system(eng, *_case_system(name), C)
    assert eng.stats()["counts"]["lu_fallback"] == 0


@pytest.mark.parametrize("n,m,p", SHAPES)
def test_one_trial_matches_the_full_record(n, m, p):
    eng = _engine(_scene(n, m, p), "compact")
    info = eng.schur_info()
    assert info["slot_rows"] % 64 == 0 and info["slot_rows"] > info["items"]  # (padding rows: the last step of a list is partly filled)
    _same_step(_trial(eng), _full_trial(n, m, p))


def test_two_compact_engines_are_bitwise_identical():
    sc = _scene(3000, 30, 0.3)
    a, b = _trial(_engine(sc, "compact")), _trial(_engine(sc, "compact"))
    for k in ("A", "b", "dxi", "tX"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_debug_reads_expand_the_compact_record():
    """residual and J_X are the values K1 stores in either layout: bit for bit.  J_C: f, u, v, t columns bit for bit, the omega
    columns are (row of J_X) x (X - t) on the host against K1's own -- 1e-12 of the largest entry of J_C (a cross product
    cancels: an entry far below the operands' products carries their rounding, not its own)."""
    sc = _scene(3000, 12, 0.5)
    c, f = _engine(sc, "compact"), _engine(sc, "full")
    c.linearize(), f.linearize()
    np.testing.assert_array_equal(c.debug_read("residual"), f.debug_read("residual"))
    np.testing.assert_array_equal(c.debug_read("JX"), f.debug_read("JX"))
    for k in ("E", "dP"):
        np.testing.assert_array_equal(c.debug_read(k), f.debug_read(k), err_msg=k)  # K2's sums: unchanged, bit for bit
    Jc, Jf = c.debug_read("JC").reshape(-1, 2, 9), f.debug_read("JC").reshape(-1, 2, 9)
    np.testing.assert_array_equal(Jc[:, :, :6], Jf[:, :, :6])
    dev = np.abs(Jc - Jf).max() / np.abs(Jf).max()
    print(f"J_C compact vs full: max|d| / max|J_C| = {dev:.3e} (bound 1e-12)")
    assert np.abs(Jf[:, :, 6:]).max() > 0 and dev <= 1e-12


def test_covariances_match_the_full_record():
    """mvba_covariance on a compact engine (its point pass reads full-layout records of a second K1 launch) against the full
    engine's.  The two engines' undamped S differ at rounding level and S^-1 amplifies that by cond(S): the bound
    tests/test_gpu_covariance.py has for results from differently rounded S, 1e-7 of the largest entry (1e-8 is its bound
    against a reference built from the engine's OWN S)."""
    sc = _scene(3000, 12, 0.5)
    got, ref = _engine(sc, "compact").covariance(full=True), _engine(sc, "full").covariance(full=True)
    for k in ("points", "cameras", "cameras_full"):
        dev = np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max()
        print(f"covariance {k}: compact vs full {dev:.3e} (bound 1e-7)")
        assert dev <= 1e-7, k


@functools.lru_cache(maxsize=None)
def _wide_case():
    """1500 x 80 at 10 %, points 0, 700 and 1499 seen by all 80 cameras: more than 64 observations, K1's split tiles."""
    n, m = 1500, 80
    sc = make_scene(n, m, vis_p=1.0, project="numpy")
    keep = np.random.default_rng(V.SEED).random((n, m)) < 0.1
    keep[[0, 700, 1499]] = True
    keep[keep.sum(1) < 2, :2] = True
    return sc, V.masked(sc, keep)


def test_points_seen_by_more_than_64_cameras():
    sc, obs = _wide_case()
    assert np.diff(obs[0]).max() == 80
    c, f = _engine(sc, "compact", obs), _engine(sc, "full", obs)
    got = _trial(c)
    _same_step(got, _trial(f))
    A, b, E1o = _oracle_system(_oracle(sc, *obs))
    np.testing.assert_allclose(got["A"], A, rtol=0, atol=1e-11 * np.abs(A).max())
    np.testing.assert_allclose(got["b"], b, rtol=0, atol=1e-9 * np.abs(b).max())
    assert got["E1"] == pytest.approx(E1o, rel=1e-7)


def test_held_points():
    """Every seventh point held: its row of PB is zeros but X_a (the omega columns of its observations still enter c diag G_k),
    its step exactly 0."""
    sc = _scene(3000, 30, 0.3)
    mask = np.arange(sc.n_points) % 7 == 3
    c, f = _engine(sc, "compact"), _engine(sc, "full")
    c.set_point_hold(mask), f.set_point_hold(mask)
    got = _trial(c)
    _same_step(got, _trial(f))
    assert (got["dX"][mask] == 0).all() and (got["dX"][~mask] != 0).any()


def test_hold_only_parameter_map():
    sc = _scene(3000, 30, 0.3)
    col, n_free = parameter_map(sc.n_images, sc.axis, hold="intrinsics")
    c, f = _engine(sc, "compact"), _engine(sc, "full")
    c.set_parameter_map(col, n_free), f.set_parameter_map(col, n_free)
    got = _trial(c)
    _same_step(got, _trial(f))
    assert (got["dxi"].reshape(-1, 9)[:, :3] == 0).all()


def test_two_thread_ranks_host_transport():
    """Sharded engines in the lane form (as tests/test_gpu_covariance.py::test_two_thread_ranks_host_transport shards: two ranks
    as threads over the host transport, partition_points / slice_observations), every rank on the compact record: one trial's
    summed [A | b] on rank 0 against the single compact engine's, both ranks' dxi bit for bit equal, and the single engine
    against the oracle (check_reduced_system).  Bounds: the ranks sum the same items as the single engine in another order -- per
    rank in list order, then over the ranks -- which is what _same_step's bounds are for (two engines, each within the oracle
    bound of 1e-11 max|A| and 1e-9 max|b|, so 2e-11 and 2e-9 between them; tests/test_gpu_schur_lanes.py compares k_schur_lanes
    with k_schur_slots at the same)."""
    from lib import _distributed as D
    from lib._mvba import HipEngine
    from oracle import ba_oracle as O

    n, m, p = 3000, 30, 0.3
    sc = _scene(n, m, p)
    X, R, t = O.normalize_scene(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    f, u = sc.init_K[:, 0, 0].copy(), sc.init_K[:, :2, 2].copy()
    one = _engine(sc, "compact")
    check_reduced_system(one, *_oracle_system(_oracle(sc)), C)
    ref = _trial(one)
    parts = D.partition_points(sc.pt_ptr, 2)

    def body(rank, g):
        lo, hi = parts[rank]
        p2, c2, x2 = D.slice_observations(sc.pt_ptr, sc.cam_idx, sc.xy, lo, hi)
        eng = HipEngine(hi - lo, m, p2, c2, x2, 1.0, sc.axis)  # (MVBA_SCHUR=lanes is set around the whole group: one environment)
        info = eng.schur_info()
        assert info["kernel"] == "slots" and info["step_width"] == 64 and info["record"] == "compact", info
        g.attach(eng, rank)
        eng.set_params(X[lo:hi], f, u, t, R)
        return _trial(eng), info

    with _env(MVBA_SCHUR="lanes"):
        res = D.InProcessGroup(2).run(body)
    for rank, (_, info) in enumerate(res):
        print(f"rank {rank}: points {parts[rank]}, form {info['kernel']}, step width {info['step_width']}, record {info['record']}")
    got = res[0][0]
    dev_A, dev_b = np.abs(got["A"] - ref["A"]).max() / np.abs(ref["A"]).max(), np.abs(got["b"] - ref["b"]).max() / np.abs(ref["b"]).max()
    print(f"two ranks vs one engine: |dA| / max|A| = {dev_A:.3e} (2e-11), |db| / max|b| = {dev_b:.3e} (2e-9), trial cost rel. "
          f"{abs(got['E1'] - ref['E1']) / ref['E1']:.3e} (1e-9)")
    assert dev_A <= 2e-11 and dev_b <= 2e-9
    assert got["E1"] == pytest.approx(ref["E1"], rel=1e-9)
    np.testing.assert_array_equal(res[0][0]["dxi"], res[1][0]["dxi"])
    np.testing.assert_array_equal(res[0][0]["A"], res[1][0]["A"])
    assert np.abs(got["dxi"]).max() > 0


def test_snapshot_restore_then_a_step():
    """The state of a snapshot restored after an accepted step: the next linearisation and trial are those of the first, bit
    for bit (K3a takes X_a for the point rows from the restored state, K3 the centres), and residuals() is the debug read."""
    sc = _scene(3000, 30, 0.3)
    eng = _engine(sc, "compact")
    eng.snapshot()
    first = _trial(eng)
    # (f0 = 1; two kernels evaluate one formula: check_one_step's bound on a residual)
    np.testing.assert_allclose(eng.residuals(), eng.debug_read("residual").reshape(-1, 2), rtol=1e-12, atol=1e-14)
    eng.commit()
    moved = _trial(eng)
    assert np.abs(moved["b"] - first["b"]).max() > 0
    eng.snapshot_restore(0)
    again = _trial(eng)
    for k in ("A", "b", "dxi", "tX"):
        np.testing.assert_array_equal(again[k], first[k], err_msg=k)
    assert again["E1"] == first["E1"]
