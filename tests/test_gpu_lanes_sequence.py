"""The lane-form Schur engines (k_schur_lanes on the full record, k_schur_lanes_compact with k_resid_jac<.., CompactRec> and
k_point_inv's X_a in slots 6-7 of the point row) past their first step: retries on one linearisation, linearisations after
one and two commits, five LM iterations, a state uploaded into a live engine -- at f0 = 1 and at f0 = 600.  The checks are
those of tests/_lanes_sequence.py, shown on the CPU to hold and to be able to fail by tests/test_lanes_sequence_cpu.py.

Every engine is forced into the lane form (MVBA_SCHUR=lanes; MVBA_REC=full for the full record) and asserts it:
kernel "slots", step width 64 and the record.  Shape: 3000 x 30 x 0.3, nine waves of 64 lists per range.  The f0 = 600 case
is tests/_pixel_cases.py::pixel_problem, the f0 = 1 case its unit twin (the same scene, principal points off the centre);
every comparison is on the column-scaled values (D: f0 at f, u, v), which at f0 = 1 are the values themselves.

Bounds, none of them new: tests/_parity_checks.py::check_reduced_system (A 1e-11 max|A|, b 1e-9 max|b|, trial cost 1e-7) and
check_one_step (residual .. dP, A 1e-12, b 1e-10, dxi and dX 1e-9, the trial state 1e-10, the trial cost 1e-9), as
tests/test_gpu_schur_lanes.py and tests/test_gpu_pixel_units.py::test_oracle_at_600_in_every_form hold an engine to at its
first step; the oracle is seated on the engine's own committed state before each, so nothing is added for drift.  The five
iterations: tests/test_gpu_schur_lanes.py::test_default_selection_short_run_matches_the_oracle (equal solve counts, RMSE 1e-9)."""
import functools

import numpy as np
import pytest

from _lanes_sequence import C_FIRST, commit_sequence, retry_on_one_linearisation
from _parity_checks import check_one_step
from _pixel_cases import make_engine, pixel_problem
from lib.bundle_adjustment import lm_loop
from oracle import ba_oracle as O

pytestmark = pytest.mark.gpu

SHAPE = (3000, 30, 0.3)
CASES = [(rec, f0) for rec in ("compact", "full") for f0 in (1.0, 600.0)]
case = pytest.mark.parametrize("record,f0", CASES, ids=[f"{r}-f0_{f0:g}" for r, f0 in CASES])


@functools.lru_cache(maxsize=None)
def _problem(f0):
    px, twin, D = pixel_problem(*SHAPE, 600.0)
    return (px, D) if f0 == 600.0 else (twin, np.ones_like(D))


def _lanes_engine(monkeypatch, prob, record):
    """A HipEngine on `prob` in the lane form on `record`; a fall-back to k_schur_slots or to the other record fails here."""
    from lib._mvba import HipEngine

    monkeypatch.setenv("MVBA_SCHUR", "lanes")
    if record == "full":
        monkeypatch.setenv("MVBA_REC", "full")
    else:
        monkeypatch.delenv("MVBA_REC", raising=False)
    eng = make_engine(HipEngine, prob)
    info = eng.schur_info()
    assert info["kernel"] == "slots" and info["step_width"] == 64 and info["record"] == record, info
    print(f"{SHAPE} f0 = {prob[5]:g}: form {info['kernel']}, step width {info['step_width']}, record {info['record']}")
    return eng


@case
def test_retries_on_one_linearisation(monkeypatch, record, f0):
    """linearize(), then try_step at 1e-4, 1e-1 and 1e-4 again with nothing committed (the LM retry): each trial against the
    oracle's at that damping; the linearisation untouched by the trials and the repeated trial equal to the first, bit for bit."""
    prob, D = _problem(f0)
    retry_on_one_linearisation(_lanes_engine(monkeypatch, prob, record), make_engine(O.OracleEngine, prob), D)


@case
def test_linearisations_after_one_and_two_commits(monkeypatch, record, f0):
    """One step at the uploaded state, commit, the oracle seated on the engine's committed state, one step; and once more: the
    current-state buffer (where k_point_inv takes X_a from) and the committed camera table (the centres) have each been both of
    their two.  b_full moves by more than its bound between the states, so a stale linearisation cannot pass."""
    prob, D = _problem(f0)
    commit_sequence(_lanes_engine(monkeypatch, prob, record), make_engine(O.OracleEngine, prob), D, n_commits=2)


@case
def test_five_lm_iterations_match_the_oracle(monkeypatch, record, f0):
    prob, D = _problem(f0)
    eng, g = _lanes_engine(monkeypatch, prob, record), make_engine(O.OracleEngine, prob)
    eng.n_solves = g.n_solves = 0
    Eg = lm_loop(eng, 2.0, -1.0, 5, verbose=False)
    Eo = lm_loop(g, 2.0, -1.0, 5, verbose=False)
    n_obs = eng.n_obs
    dev = abs(np.sqrt(Eg / n_obs) - np.sqrt(Eo / n_obs))
    print(f" five LM iterations: solves {eng.n_solves} (oracle {g.n_solves}), |RMSE - oracle's| = {dev:.3e} (bound 1e-9), "
          f"LU rescues {eng.stats()['counts']['lu_fallback']}")
    assert eng.n_solves == g.n_solves
    assert dev < 1e-9
    assert eng.stats()["counts"]["lu_fallback"] == 0


@pytest.mark.parametrize("f0", [1.0, 600.0])
def test_a_state_uploaded_into_a_live_compact_engine(monkeypatch, f0):
    """set_params on an engine that has linearised, stepped and committed (its current buffer is the second one): the next step
    against an oracle at the uploaded state -- the point rows (X_a) and the centres must come from the upload.  The uploaded
    state is the oracle's after one accepted step from the first, so it differs from both states the engine has held."""
    prob, D = _problem(f0)
    eng, g = _lanes_engine(monkeypatch, prob, "compact"), make_engine(O.OracleEngine, prob)
    eng.linearize()
    eng.try_step(1e-2)
    eng.commit()
    held = eng.get_params()
    g.linearize()
    g.try_step(C_FIRST)
    g.commit()
    state = g.get_params()
    for a, b0, b1 in zip(state, prob[7:], held):
        assert not np.array_equal(a, b0) and not np.array_equal(a, b1)
    eng.set_params(*state)
    for a, b in zip(eng.get_params(), state):
        assert np.array_equal(a, b)
    check_one_step(eng, g, C_FIRST, col_scale=D)
    assert eng.stats()["counts"]["lu_fallback"] == 0
