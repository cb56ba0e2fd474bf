"""The method of tests/_lanes_sequence.py on the CPU: it holds on a correct engine (the oracle behind the device protocol, at
f0 = 1 and in pixel units), and it can fail -- an engine whose omega columns come from the points and centres of the first
state it saw (``StaleOmegaOracle``) is the oracle BIT FOR BIT in the one-trial check at the uploaded state, which is all the
suite asked of the lane-form engines before tests/test_gpu_lanes_sequence.py, and fails the check after one commit at the
same bounds.  Also measured here: why no part of the reduced matrix is shared between two dampings."""
import numpy as np
import pytest

from _lanes_sequence import (C_FIRST, C_RETRY, TRIAL, OracleAsDevice, StaleOmegaOracle, commit_sequence, retry_on_one_linearisation,
                             step_after_commit)
from _parity_checks import check_one_step
from _pixel_cases import make_engine, pixel_problem
from oracle import ba_oracle as O

SHAPE = (300, 8, 0.5)  # (tests/test_pixel_units_cpu.py::SHAPES[0])


def _problem(f0):
    """The pixel problem at f0 = 600, or its unit twin (f0 = 1, principal points off the centre all the same)."""
    px, twin, D = pixel_problem(*SHAPE, 600.0)
    return (px, D) if f0 == 600.0 else (twin, np.ones_like(D))


@pytest.mark.parametrize("f0", [1.0, 600.0])
def test_the_sequence_checks_hold_on_a_correct_engine(f0):
    prob, D = _problem(f0)
    eng, g = OracleAsDevice(make_engine(O.OracleEngine, prob)), make_engine(O.OracleEngine, prob)
    retry_on_one_linearisation(eng, g, D)
    commit_sequence(eng, g, D)


@pytest.mark.parametrize("f0", [1.0, 600.0])
def test_a_stale_point_row_or_centre_shows_after_a_commit_and_not_before(f0):
    prob, D = _problem(f0)
    good, bad = OracleAsDevice(make_engine(O.OracleEngine, prob)), OracleAsDevice(make_engine(StaleOmegaOracle, prob))
    g = make_engine(O.OracleEngine, prob)
    # the gap: one linearisation and one trial at the uploaded state, every output bit for bit the oracle's
    check_one_step(bad, g, C_FIRST, col_scale=D)
    check_one_step(good, g, C_FIRST, col_scale=D)
    for k in ("JC",) + TRIAL:
        assert np.array_equal(bad.debug_read(k), good.debug_read(k)), k
    # ... and so is a retry on that linearisation
    retry_on_one_linearisation(bad, g, D)
    # after one commit the same check, at the same bounds, fails -- on J_C itself and on what is built from it
    bad.try_step(C_FIRST)
    with pytest.raises(AssertionError):
        step_after_commit(bad, g, D)
    JC, JC_ref = bad.debug_read("JC").reshape(-1, 2, 9), g.JC
    assert np.array_equal(JC[:, :, :6], JC_ref[:, :, :6])  # (only the omega columns are stale)
    dev = np.abs(JC - JC_ref).max() / np.abs(JC_ref).max()
    print(f"stale omega columns after one commit: max|dJ_C| / max|J_C| = {dev:.3e} (check_one_step's bound: 1e-12)")
    assert dev > 1e-9
    # the correct engine passes the very call that the mutant failed
    good.try_step(C_FIRST)
    step_after_commit(good, g, D)


def test_no_part_of_the_reduced_matrix_is_shared_between_two_dampings():
    """A(c) = G + c diag(G) - F^T (E + c diag E)^-1 F: with the term c diag(G) taken off, the matrices of c = 1e-4 and c = 1e-1
    still differ by a fraction of max|A| that is no rounding -- the damping of E_a reaches every entry.  So
    retry_on_one_linearisation asks for bitwise equality of a REPEATED trial, not of A(c) - c diag(G) across dampings."""
    prob, _ = _problem(1.0)
    g = make_engine(O.OracleEngine, prob)
    g.linearize()
    rest = []
    for c in (C_FIRST, C_RETRY):
        A, _ = g.reduced_system(c)
        for k in range(g.m):
            A[9 * k:9 * k + 9, 9 * k:9 * k + 9] -= c * np.diag(np.diag(g.G[k]))
        rest.append(A)
    dev = np.abs(rest[0] - rest[1]).max() / np.abs(rest[0]).max()
    print(f"A(c) - c diag(G) at c = {C_FIRST:g} against c = {C_RETRY:g}: max|diff| / max|A| = {dev:.3e}")
    assert dev > 1e-6
