"""The one-step comparisons of a HIP engine with the oracle that several GPU test files share, tolerances written at each assert.
Test infrastructure only."""
import numpy as np
import pytest


def _scaled(col_scale, m):
    """The column scale as a checked (9m,) vector -- f0 at (f, u, v) of every camera, 1 at the pose slots -- or None."""
    if col_scale is None:
        return None
    D = np.asarray(col_scale, np.float64).reshape(-1)
    assert D.shape == (9 * m,) and (D.reshape(m, 9) == D[:9]).all() and (D[:3] == D[0]).all() and (D[3:9] == 1.0).all()
    return D


def check_one_step(eng, g, c, tight=1e-11, col_scale=None, dxi_tol=1e-9, linearize=True):
    """Every kernel's output at one linearisation point + one trial.  ``col_scale`` (9m,): the vector D of a problem in
    pixel units (tests/_pixel_cases.py), f0 at (f, u, v) and 1 at the pose slots: JC, A_full, b_full, dxi and the trial
    f, u of the engine AND of the oracle go to the unit twin's scale (JC D, D A D, D b, dxi / D, f / f0, u / f0) before the
    same asserts with the same numbers -- unscaled, the f / u block of A is f0^2 below max|A| and a bound relative to
    max|A| does not see it.  ``dxi_tol``: the bound on dxi as a fraction of max|dxi|, 1e-9 unless the caller has a written reason
    (tests/_pixel_cases.py::ORACLE_TWIN_DXI: the ORACLE's LU solve of the unscaled system at 647 cameras).
    ``linearize=False``: both are linearised at one state already and stay so -- a further trial on that linearisation (the LM
    retry, tests/_lanes_sequence.py); the linearisation is read and compared all the same, the committed cost is not asked for."""
    D = _scaled(col_scale, g.m)
    d9, f0 = (1.0, 1.0) if D is None else (D[:9], D[0])
    Dv = 1.0 if D is None else D
    DD = 1.0 if D is None else np.outer(D, D)
    if linearize:
        assert eng.cost() == pytest.approx(g.cost(), rel=1e-13)
        eng.linearize()
        g.linearize()
    n_obs = g.xy.shape[0]
    np.testing.assert_allclose(eng.debug_read("residual").reshape(n_obs, 2), g.e, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(eng.debug_read("JX").reshape(n_obs, 2, 3), g.JX, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(eng.debug_read("JC").reshape(n_obs, 2, 9) * d9, g.JC * d9, rtol=1e-12, atol=1e-12)
    E6 = eng.debug_read("E").reshape(-1, 6)
    iu = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])
    np.testing.assert_allclose(E6, g.E[:, iu[0], iu[1]], rtol=tight, atol=1e-12 * np.abs(g.E).max())
    # dP_a = 2 sum J^T e cancels near a minimum: bound by 1e-12 x (sum of |terms|)
    dP_scale = 2 * np.abs(g.JX).max() * np.abs(g.e).max() * np.diff(g.pt_ptr).max()
    np.testing.assert_allclose(eng.debug_read("dP").reshape(-1, 3), g.dP, rtol=tight, atol=1e-12 * dP_scale)
    E1 = eng.try_step(c)
    A, b = g.reduced_system(c)
    E1o = g.try_step(c)
    m9 = 9 * g.m
    Agpu = eng.debug_read("A_full").reshape(m9, m9) * DD
    A, b = A * DD, b * Dv
    sc = np.abs(A).max()
    if D is not None:
        print(f"  one step, scaled by D (f0 = {f0:g}): |dA| / max|A| = {np.abs(Agpu - A).max() / sc:.3e} (bound 1e-12), |db| / max|b| = "
              f"{np.abs(eng.debug_read('b_full') * Dv - b).max() / np.abs(b).max():.3e} (bound 1e-10), |ddxi| / max|dxi| = "
              f"{np.abs(eng.debug_read('dxi')[g.keep] / D[g.keep] - g.dxi_red / D[g.keep]).max() / np.abs(g.dxi_red / D[g.keep]).max():.3e} "
              f"(bound {dxi_tol:g}), |ddX| / max|dX| = {np.abs(eng.debug_read('dX').reshape(-1, 3) - g.dX).max() / np.abs(g.dX).max():.3e} (bound 1e-9)")
    np.testing.assert_allclose(Agpu, A, rtol=0, atol=1e-12 * sc)
    # b = sum_a F^T E^-1 dP - dF is a difference of two much larger sums: 1e-10 of max|b|
    np.testing.assert_allclose(eng.debug_read("b_full") * Dv, b, rtol=0, atol=1e-10 * np.abs(b).max())
    dxi = np.zeros(m9)
    dxi[g.keep] = g.dxi_red
    dxi = dxi / Dv
    np.testing.assert_allclose(eng.debug_read("dxi") / Dv, dxi, rtol=0, atol=dxi_tol * np.abs(dxi).max())
    assert (eng.debug_read("dxi")[g.removed] == 0).all()
    np.testing.assert_allclose(eng.debug_read("dX").reshape(-1, 3), g.dX, rtol=0, atol=1e-9 * np.abs(g.dX).max())
    np.testing.assert_allclose(eng.debug_read("trial_X").reshape(-1, 3), g.tX, rtol=0, atol=1e-10)
    tc = eng.debug_read("trial_cam").reshape(g.m, 15)
    np.testing.assert_allclose(tc[:, 0] / f0, g.tf / f0, atol=1e-10)
    np.testing.assert_allclose(tc[:, 1:3] / f0, g.tu / f0, atol=1e-10)
    np.testing.assert_allclose(tc[:, 3:6], g.tt, atol=1e-10)
    np.testing.assert_allclose(tc[:, 6:].reshape(-1, 3, 3), g.tR, atol=1e-10)
    assert E1 == pytest.approx(E1o, rel=1e-9, abs=1e-13)
    return E1


def check_reduced_system(eng, A, b, E1o, c=1e-2, col_scale=None, linearize=True):
    """One linearisation and one trial at damping c on `eng` against the oracle's reduced system (A, b) and trial cost E1o at the
    same state and damping: A_full to 1e-11 max|A|, b_full to 1e-9 max|b|, the trial cost to 1e-7 relative.  Returns the measured
    max|A_full - A| / max|A|.  ``col_scale``: as for check_one_step, D A D and D b on both sides first.  ``linearize=False``: the
    trial alone, on the linearisation `eng` already has."""
    if linearize:
        eng.linearize()
    E1 = eng.try_step(c)
    m9 = A.shape[0]
    D = _scaled(col_scale, m9 // 9)
    Agpu, bgpu = eng.debug_read("A_full").reshape(m9, m9), eng.debug_read("b_full")
    if D is not None:
        A, b, Agpu, bgpu = A * np.outer(D, D), b * D, Agpu * np.outer(D, D), bgpu * D
    dev_A, dev_b = np.abs(Agpu - A).max() / np.abs(A).max(), np.abs(bgpu - b).max() / np.abs(b).max()
    print(f"reduced system vs oracle: |dA| / max|A| = {dev_A:.3e} (bound 1e-11), |db| / max|b| = {dev_b:.3e} (bound 1e-9), "
          f"trial cost rel. {abs(E1 - E1o) / abs(E1o):.3e} (bound 1e-7)")
    np.testing.assert_allclose(Agpu, A, rtol=0, atol=1e-11 * np.abs(A).max())
    np.testing.assert_allclose(bgpu, b, rtol=0, atol=1e-9 * np.abs(b).max())
    assert E1 == pytest.approx(E1o, rel=1e-7)
    return dev_A
