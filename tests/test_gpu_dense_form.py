"""k_schur_dense (csrc/mvba_dense.h) against the oracle where its compile-time decisions differ: at every tile count T = 2 .. 12
(pair-to-wave tables, role split, chunk size, prefetch depth), contiguous and through the (point, camera) table, squared and
Huber; past the second chunk of a workgroup (both loop halves in steady state, both exits, every re-fetched set); and at a
negative damping that gives the points MIXED sign codes.  Cases, launch rule and references: tests/_dense_cases.py; that the
cases reach all this: tests/test_dense_cases_cpu.py."""
import numpy as np
import pytest

import _dense_cases as D
from _parity_checks import check_reduced_system

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def n_cu():
    """The device's compute units, read off a launch with more chunks than the device takes workgroups: two cameras (T = 2, two
    workgroups per CU) x 16 384 points = 4 096 chunks.  It is the one launch this file does not hold to the restated rule; every
    other one -- all tile counts, both workgroups-per-CU values, both chunk sizes, saturated or not -- is held to it with this
    count.  (torch would give the count too, but needs its own HIP runtime initialised in a process in which the library's
    already is: not in one run with the rest of the suite.)"""
    from lib._mvba import HipEngine

    n, m, pt_ptr, cam, xy, f0, axis, *state = D.problem(D.Case(16384, 2, 1.0, "squared"))
    eng = HipEngine(n, m, pt_ptr, cam, xy, f0, axis)
    info = eng.schur_info()
    eng.close()
    W, per_cu = info["workgroups"], D.workgroups_per_cu(D.tiles(2))
    assert info["kernel"] == "dense" and 2 * per_cu <= W < D.launch(n, m, 1 << 20)[3] and W % per_cu == 0, info
    return W // per_cu


def _engine(case, n_cu):
    """The HIP engine on the case, in the dense form with the launch the restated rule gives for this device."""
    from lib._mvba import HipEngine

    n, m, pt_ptr, cam, xy, f0, axis, *state = D.problem(case)
    eng = HipEngine(n, m, pt_ptr, cam, xy, f0, axis, **D.engine_kwargs(case))
    eng.set_params(*state)
    info = eng.schur_info()
    assert info["kernel"] == "dense"
    assert info["workgroups"] == D.launch(n, m, n_cu)[2], (info, D.launch(n, m, n_cu))
    return eng, info


def _rel(a, b):
    return float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())


def _huber_trial(eng, ref):
    """tests/test_gpu_robust.py::_check_step's bounds: A_full and b_full to 1e-10 of their largest entry, the trial cost to 1e-9."""
    eng.linearize()
    E1 = eng.try_step(D.C)
    m9 = ref.A.shape[0]
    dA, db = _rel(eng.debug_read("A_full").reshape(m9, m9), ref.A), _rel(eng.debug_read("b_full"), ref.b)
    print(f"reduced system vs robust reference: |dA| / max|A| = {dA:.3e} (bound 1e-10), |db| / max|b| = {db:.3e} (bound 1e-10), "
          f"trial cost rel. {abs(E1 - ref.E1) / abs(ref.E1):.3e} (bound 1e-9)")
    assert dA <= 1e-10 and db <= 1e-10
    assert E1 == pytest.approx(ref.E1, rel=1e-9)
    return dA


def _sign_trial(eng, ref):
    """One more trial on the linearisation `eng` has, at the case's SIGN_C: A_full within MARGIN x the case's host-versus-host figure
    (floor: 1e-11 max|A|), b_full as in check_reduced_system, dxi and the trial cost within the bounds of
    tests/test_gpu_parity.py::test_indefinite_reduced_system_takes_the_lu_path_like_numpy (1e-8 max|dxi|, 1e-6), one more LU solve."""
    lu = eng.stats()["counts"]["lu_fallback"]
    E1 = eng.try_step(ref.sign_c)
    m9 = ref.A_s.shape[0]
    bound = D.sign_bound(ref.host_diff_s)
    dA, db = _rel(eng.debug_read("A_full").reshape(m9, m9), ref.A_s), _rel(eng.debug_read("b_full"), ref.b_s)
    ddxi = _rel(eng.debug_read("dxi"), ref.dxi_s)
    print(f"SIGN_C {ref.sign_c}: |dA| / max|A| = {dA:.3e} (bound {bound:.1e}: host versus host {ref.host_diff_s:.1e}), |db| / max|b| = "
          f"{db:.3e} (bound 1e-9), |ddxi| / max|dxi| = {ddxi:.3e} (bound 1e-8), trial cost rel. {abs(E1 - ref.E1_s) / abs(ref.E1_s):.3e} (bound 1e-6)")
    assert ref.eig_s[0] < 0 < ref.eig_s[1]
    assert dA <= bound and db <= 1e-9 and ddxi <= 1e-8
    assert E1 == pytest.approx(ref.E1_s, rel=1e-6)
    assert eng.stats()["counts"]["lu_fallback"] == lu + 1
    return dA


@pytest.mark.parametrize("m", list(D.SWEEP))
def test_every_tile_count_matches_the_oracle(m, n_cu, monkeypatch):
    """One camera count per test, m = 2 .. 21 (T = 2 .. 12): every size of the case contiguous and through the table, squared
    (check_reduced_system, then one trial at SIGN_C on the same linearisation) and Huber."""
    monkeypatch.setenv("MVBA_SCHUR", "dense")
    T = D.tiles(m)
    for case in D.sweep_cases(m):
        eng, info = _engine(case, n_cu)
        ref = D.reference(case)
        row = (f"dense sweep m = {m:2d}  T = {T:2d}  CH = {D.chunk_points(T)}  consumers = {D.consumers(T)}  NPRE = {D.npre(T)}  "
               f"N = {case.n:3d}  {'contiguous' if case.vis >= 1.0 else 'table     '}  {case.loss:7s}  workgroups = {info['workgroups']:2d}")
        if case.loss == "squared":
            dA = check_reduced_system(eng, ref.A, ref.b, ref.E1, c=D.C)
            dA_s = _sign_trial(eng, ref)
            print(f"{row}  |dA| / max|A| = {dA:.3e}  at SIGN_C {ref.sign_c}: {dA_s:.3e}")
        else:
            dA = _huber_trial(eng, ref)
            print(f"{row}  |dA| / max|A| = {dA:.3e}")
        eng.close()


@pytest.mark.parametrize("table", [False, True], ids=["contiguous", "table"])
@pytest.mark.parametrize("m", list(D.DEPTH))
def test_workgroups_of_many_chunks_match_the_oracle(m, table, n_cu, monkeypatch):
    """N from this device's workgroup count W so that n_chunks = 2 W + r and 6 W + r, 0 < r < W: workgroups of 3 | 2 and of
    7 | 6 chunks -- the set re-fetched after the first build, both loop halves in steady state, both exits, the consumers'
    buffer parity past the second chunk, the table row fetched four ahead.  The premise is asserted from the launch the engine
    reports.  A chunk lost, built twice or read from the stale buffer moves A by about CH / N ~ 3e-4 of its size."""
    monkeypatch.setenv("MVBA_SCHUR", "dense")
    for q in D.DEPTH_Q:
        case = D.depth_case(m, q, table, n_cu)
        eng, info = _engine(case, n_cu)
        T, CH, _, n_chunks = D.launch(case.n, m, n_cu)
        W = info["workgroups"]
        r = n_chunks - (q - 1) * W
        assert 0 < r < W and case.n % CH != 0, (case, W, n_chunks)
        per = D.chunks_per_workgroup(n_chunks, W)
        assert per == {q: r, q - 1: W - r}
        print(f"dense depth m = {m}  T = {T}  CH = {CH}  NPRE = {D.npre(T)}  {'table' if table else 'contiguous'} ({case.vis:g})  "
              f"N = {case.n}  W = {W}  n_chunks = {n_chunks} = {q - 1} W + {r}  chunks per workgroup: {per}")
        ref = D.reference(case, sign=not table)
        check_reduced_system(eng, ref.A, ref.b, ref.E1, c=D.C)
        if not table:
            _sign_trial(eng, ref)
        eng.close()
