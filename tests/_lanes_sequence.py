"""An engine past its first step: several trials on one linearisation (the LM retry), linearisations after commits, a state
uploaded into a live engine -- each against the oracle seated on the engine's OWN committed state, so that both linearise at
bit-identical numbers and the one-step bounds of tests/_parity_checks.py apply without an allowance for two trajectories
drifting apart.  Test infrastructure only; used by tests/test_gpu_lanes_sequence.py on the lane-form engines and by
tests/test_lanes_sequence_cpu.py, which shows on the CPU that the method holds on a correct engine and can fail.

Why this exists: k_schur_lanes_compact forms the omega columns of J_C from X_a (slots 6-7 of the point row, which
k_point_inv copies from the CURRENT state buffer) and from the centres in the committed camera table.  At the state
set_params uploaded, a kernel that read the other buffer, or a table that a commit did not refresh, computes the right
numbers; only a linearisation after a commit tells them apart (``StaleOmegaOracle`` is that engine)."""
import numpy as np

from _parity_checks import check_one_step, check_reduced_system
from oracle import ba_oracle as O

C_FIRST, C_RETRY = 1e-4, 1e-1  # the two dampings of a rejected and repeated trial (tests/test_gpu_constraints.py uses the same pair)
LINEARISATION = ("residual", "JX", "JC", "E", "dP")
TRIAL = ("A_full", "b_full", "dxi", "dX", "trial_X", "trial_cam")


def _oracle_trial(g, c):
    """(A, b, E1o) of the linearised oracle at damping c -- what check_reduced_system takes."""
    A, b = g.reduced_system(c)
    return A, b, g.try_step(c)


def retry_on_one_linearisation(eng, g, D):
    """linearize() once, then trials at C_FIRST, C_RETRY and C_FIRST again, nothing committed.  Each trial: check_reduced_system's
    bounds on A_full, b_full and the trial cost, check_one_step's on the linearisation, dxi, dX and the trial state.

    What must not depend on the trials before it holds BIT FOR BIT: the five arrays of the linearisation after every trial, and
    everything the third trial computed against the first (the same damping on the same linearisation).  The reduced matrices of
    two DIFFERENT dampings have no part that is equal: c enters E^-1 = (E + c diag E)^-1 and through it every entry of
    F^T E^-1 F, not only the term c diag(G) (tests/test_lanes_sequence_cpu.py measures this on the oracle)."""
    eng.linearize()
    g.linearize()
    lin = {k: eng.debug_read(k) for k in LINEARISATION}
    first = None
    for i, c in enumerate((C_FIRST, C_RETRY, C_FIRST)):
        print(f" trial {i} on one linearisation, c = {c:g}")
        check_reduced_system(eng, *_oracle_trial(g, c), c, col_scale=D, linearize=False)
        E1 = check_one_step(eng, g, c, col_scale=D, linearize=False)
        for k in LINEARISATION:
            assert np.array_equal(eng.debug_read(k), lin[k]), (k, "changed by a trial")
        got = {k: eng.debug_read(k) for k in TRIAL}
        if i == 0:
            first, E_first = got, E1
        elif i == 1:
            assert not np.array_equal(got["A_full"], first["A_full"]) and not np.array_equal(got["dxi"], first["dxi"])
        else:
            for k in TRIAL:
                assert np.array_equal(got[k], first[k]), (k, "a repeated trial differs from the first")
            assert E1 == E_first
    assert eng.stats()["counts"]["lu_fallback"] == 0


def step_after_commit(eng, g, D, c=C_FIRST):
    """`eng` has a trial pending: commit it, seat the oracle on the engine's committed state (get_params: bit-identical numbers
    on both sides), then one linearisation and one trial at damping c through check_reduced_system and check_one_step with
    their own bounds.  Leaves that trial pending; returns b_full scaled by D, for ``assert_moved``."""
    eng.commit()
    g.set_params(*eng.get_params())
    g.linearize()
    check_reduced_system(eng, *_oracle_trial(g, c), c, col_scale=D)
    check_one_step(eng, g, c, col_scale=D)
    assert eng.stats()["counts"]["lu_fallback"] == 0
    return eng.debug_read("b_full") * D


def assert_moved(b_new, b_old):
    """The linearisation is another one: b_full (in the twin's units) moved by more than the 1e-9 max|b| it is held to --
    a test that passed on a stale linearisation would stop here."""
    moved = np.abs(b_new - b_old).max() / np.abs(b_old).max()
    print(f" b_full moved by {moved:.3e} of max|b| between the states (more than the bound on b, 1e-9)")
    assert moved > 1e-9


def commit_sequence(eng, g, D, n_commits=2):
    """One trial at the uploaded state, then ``n_commits`` times step_after_commit: with two commits the engine's current-state
    buffer has been each of its two."""
    g.set_params(*eng.get_params())
    check_one_step(eng, g, C_FIRST, col_scale=D)
    b = [eng.debug_read("b_full") * D]
    for i in range(n_commits):
        print(f" after commit {i + 1}")
        b.append(step_after_commit(eng, g, D))
        assert_moved(b[-1], b[-2])


# ---------------------------------------------------------------- oracle engines behind the device engine's protocol (CPU tests)
class OracleAsDevice:
    """An oracle engine read the way _parity_checks reads a HipEngine: debug_read(name), stats(), try_step on the linearisation
    it has.  Wraps ``g``; nothing is computed here."""

    def __init__(self, g):
        self.g, self.m, self.n_obs = g, g.m, g.xy.shape[0]

    def set_params(self, *state):
        self.g.set_params(*state)

    def get_params(self):
        return self.g.get_params()

    def cost(self):
        return self.g.cost()

    def linearize(self):
        self.g.linearize()

    def commit(self):
        self.g.commit()

    def try_step(self, c):
        g = self.g
        self.A, self.b = g.reduced_system(c)
        self.dxi = np.array(g.solve_reduced(self.A, self.b))
        return g.apply_step(self.dxi)

    def stats(self):
        return {"counts": {"lu_fallback": 0}}

    def debug_read(self, name):
        g = self.g
        iu = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])
        out = {"residual": lambda: g.e, "JX": lambda: g.JX, "JC": lambda: g.JC, "E": lambda: g.E[:, iu[0], iu[1]], "dP": lambda: g.dP,
               "A_full": lambda: self.A, "b_full": lambda: self.b, "dxi": lambda: self.dxi, "dX": lambda: g.dX,
               "trial_X": lambda: g.tX,
               "trial_cam": lambda: np.concatenate([g.tf[:, None], g.tu, g.tt, g.tR.reshape(g.m, 9)], axis=1)}[name]()
        return np.array(out, np.float64).reshape(-1)


class StaleOmegaOracle(O.OracleEngine):
    """The oracle, but the omega columns of J_C -- (row of J_X) x (X_a - t_k) -- take X_a and t_k from the FIRST state this
    engine linearised at: a compact-record kernel that reads the point rows or the centres from a buffer no commit refreshes.
    At that first state the correction added below is exactly zero and the engine is the oracle bit for bit."""

    first = None

    def linearize(self):
        e, JX, JC = O.jacobians(self.X, self.f, self.u, self.t, self.R, self.f0, self.pt, self.cam, self.xy)
        d = self.X[self.pt] - self.t[self.cam]
        if self.first is None:
            self.first = d.copy()
        JC = JC.copy()
        JC[:, :, 6:9] += np.cross(JX, self.first[:, None, :]) - np.cross(JX, d[:, None, :])
        self.e, self.JX, self.JC = e, JX, JC
        self.dP = 2.0 * O._segsum(self.pt, np.einsum("ori,or->oi", JX, e), self.n)
        self.dF = 2.0 * O._segsum(self.cam, np.einsum("ori,or->oi", JC, e), self.m)
        self.E = 2.0 * O._segsum(self.pt, np.einsum("ori,orj->oij", JX, JX), self.n)
        self.F = 2.0 * np.einsum("ori,orj->oij", JX, JC)
        self.G = 2.0 * O._segsum(self.cam, np.einsum("ori,orj->oij", JC, JC), self.m)
