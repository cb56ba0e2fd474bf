"""The one-step comparisons of a HIP engine with the oracle that several GPU test files share, tolerances written at each assert.
Test infrastructure only."""
import numpy as np
import pytest


def check_one_step(eng, g, c, tight=1e-11):
    """Every kernel's output at one linearisation point + one trial."""
    assert eng.cost() == pytest.approx(g.cost(), rel=1e-13)
    eng.linearize()
    g.linearize()
    n_obs = g.xy.shape[0]
    np.testing.assert_allclose(eng.debug_read("residual").reshape(n_obs, 2), g.e, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(eng.debug_read("JX").reshape(n_obs, 2, 3), g.JX, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(eng.debug_read("JC").reshape(n_obs, 2, 9), g.JC, rtol=1e-12, atol=1e-12)
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
    Agpu = eng.debug_read("A_full").reshape(m9, m9)
    sc = np.abs(A).max()
    np.testing.assert_allclose(Agpu, A, rtol=0, atol=1e-12 * sc)
    # b = sum_a F^T E^-1 dP - dF is a difference of two much larger sums: 1e-10 of max|b|
    np.testing.assert_allclose(eng.debug_read("b_full"), b, rtol=0, atol=1e-10 * np.abs(b).max())
    dxi = np.zeros(m9)
    dxi[g.keep] = g.dxi_red
    np.testing.assert_allclose(eng.debug_read("dxi"), dxi, rtol=0, atol=1e-9 * np.abs(dxi).max())
    assert (eng.debug_read("dxi")[g.removed] == 0).all()
    np.testing.assert_allclose(eng.debug_read("dX").reshape(-1, 3), g.dX, rtol=0, atol=1e-9 * np.abs(g.dX).max())
    np.testing.assert_allclose(eng.debug_read("trial_X").reshape(-1, 3), g.tX, rtol=0, atol=1e-10)
    tc = eng.debug_read("trial_cam").reshape(g.m, 15)
    np.testing.assert_allclose(tc[:, 0], g.tf, atol=1e-10)
    np.testing.assert_allclose(tc[:, 1:3], g.tu, atol=1e-10)
    np.testing.assert_allclose(tc[:, 3:6], g.tt, atol=1e-10)
    np.testing.assert_allclose(tc[:, 6:].reshape(-1, 3, 3), g.tR, atol=1e-10)
    assert E1 == pytest.approx(E1o, rel=1e-9, abs=1e-13)
    return E1


def check_reduced_system(eng, A, b, E1o, c=1e-2):
    """One linearisation and one trial at damping c on `eng` against the oracle's reduced system (A, b) and trial cost E1o at the
    same state and damping: A_full to 1e-11 max|A|, b_full to 1e-9 max|b|, the trial cost to 1e-7 relative.  Returns the measured
    max|A_full - A| / max|A|."""
    eng.linearize()
    E1 = eng.try_step(c)
    m9 = A.shape[0]
    Agpu = eng.debug_read("A_full").reshape(m9, m9)
    dev_A, dev_b = np.abs(Agpu - A).max() / np.abs(A).max(), np.abs(eng.debug_read("b_full") - b).max() / np.abs(b).max()
    print(f"reduced system vs oracle: |dA| / max|A| = {dev_A:.3e} (bound 1e-11), |db| / max|b| = {dev_b:.3e} (bound 1e-9), "
          f"trial cost rel. {abs(E1 - E1o) / abs(E1o):.3e} (bound 1e-7)")
    np.testing.assert_allclose(Agpu, A, rtol=0, atol=1e-11 * np.abs(A).max())
    np.testing.assert_allclose(eng.debug_read("b_full"), b, rtol=0, atol=1e-9 * np.abs(b).max())
    assert E1 == pytest.approx(E1o, rel=1e-7)
    return dev_A
