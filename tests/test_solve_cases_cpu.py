"""The premises of tests/test_gpu_solve_sizes.py, on the oracle's reduced system (no GPU): every map of tests/_solve_cases.py
yields the order and the leading-untied count it is meant to, every mapped system is positive definite at c = 1e-4 and
indefinite at c = -1.5, the reference solution converges on all of them and agrees with a 40-digit solve where that is cheap.
Each test prints the ranges of LAPACK's own figures on these systems, the scale of the GPU tests' bounds."""
import numpy as np
import pytest

import _solve_cases as sc
from lib.bundle_adjustment import parameter_map


def test_longdouble_is_wider_than_double():
    """The residuals of omega and refined_solve need it (x87 extended: 2^-63)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -60


def test_every_map_has_its_order_and_leading_untied_count():
    axis = sc.problem44()[5]
    maps = sc.all_maps_44()
    assert {k[1] for k in maps if k[0] == "sweep"} == set(sc.SWEEP_D) | {sc.D44}
    for key, (col, n_free, want_n, want_U) in maps.items():
        assert col.shape == (9 * sc.M44,) and n_free == want_n, key
        assert sc.leading_untied(col, n_free) == want_U, key
        assert sorted(np.unique(col[col >= 0])) == list(range(n_free)), key
    dcol, dn = parameter_map(sc.M44, axis)
    for sel in sc.SELECTIONS:  # all 389 free: the default map, the engine's path without maps
        col, n_free, _, _ = maps[("sweep", sc.D44, sel)]
        assert n_free == dn and np.array_equal(col, dcol)
    for D in sc.SWEEP_D[2:]:
        assert not np.array_equal(maps[("sweep", D, "prefix")][0], maps[("sweep", D, "scatter")][0])
    for U in sc.U_SWEEP:
        col = maps[("u", U)][0]
        tied = np.nonzero(col == U)[0]
        assert list(tied) == [9 * k for k in sc.U_TIED_CAMERAS]
        untied = np.nonzero((col >= 0) & (col != U))[0]
        assert (np.diff(col[untied]) > 0).all()  # the others by ascending slot
    for size in sc.SHARE_SIZES:
        col, n_free, _, _ = maps[("share", size)]
        cnt = np.bincount(col[col >= 0], minlength=n_free)
        assert sorted(cnt[cnt > 1]) == [size] * 3 and min(64, (cnt.max() + 7) // 8) == {2: 1, 8: 1, 9: 2, 44: 6}[size]
    for m, D in sc.UNMAPPED.items():
        assert 9 * m - 7 == D


def _systems():
    """(key, c, A', b') of every system the GPU tests solve: the 44-camera maps and the engines without one."""
    g = sc.oracle_linearized(*sc.SCENE)
    maps = sc.all_maps_44()
    for c in (1e-4, -1.5):
        A, b = g.reduced_system(c)
        for key, (col, n_free, _, _) in maps.items():
            yield key, c, *sc.mapped_system(A, b, col, n_free)
    for m in sc.UNMAPPED:
        g = sc.oracle_linearized(600, m, 0.5)
        col, n_free = parameter_map(m, sc.unmapped_problem(m)[5])
        for c in (1e-4, -1.5):
            A, b = g.reduced_system(c)
            yield ("unmapped", m), c, *sc.mapped_system(A, b, col, n_free)


def test_definite_at_1e_4_indefinite_at_minus_1_5_and_the_reference_converges():
    fig = {1e-4: [], -1.5: []}
    for key, c, A, b in _systems():
        w = np.linalg.eigvalsh(A)
        x, last = sc.refined_solve(A, b)  # (raises if it does not converge)
        assert last <= sc.EPS
        x_lu = sc.lapack_lu_solve(A, b)
        if c > 0:
            assert w.min() > 0, key
            x_ch = sc.lapack_cholesky_solve(A, b)  # (LinAlgError if the factorisation meets a non-positive pivot)
            fig[c].append((sc.omega(A, b, x_ch), sc.omega(A, b, x_lu), w.min(), w.max() / w.min(),
                           sc.distance(x_ch, x) / np.abs(x_ch).max()))
        else:
            assert w.min() < 0, key
            fig[c].append((sc.omega(A, b, x_lu),))
        assert sc.omega(A, b, x) <= 2 * sc.EPS, key  # the refined solution, rounded to nothing: a residual at rounding level
    f = np.array(fig[1e-4])
    print(f"c = 1e-4, {len(f)} systems: omega Cholesky {f[:, 0].min():.1e} .. {f[:, 0].max():.1e}, omega LU {f[:, 1].min():.1e} .. "
          f"{f[:, 1].max():.1e}, min eigenvalue >= {f[:, 2].min():.1e}, cond <= {f[:, 3].max():.1e}, Cholesky to refined <= {f[:, 4].max():.1e}")
    f = np.array(fig[-1.5])
    print(f"c = -1.5, {len(f)} systems: omega LU <= {f[:, 0].max():.1e}")


def test_refined_solve_agrees_with_forty_digits_at_small_orders():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    g = sc.oracle_linearized(*sc.SCENE)
    A, b = g.reduced_system(1e-4)
    for D in (d for d in sc.SWEEP_D if d <= 33):
        for sel in sc.SELECTIONS:
            Am, bm = sc.mapped_system(A, b, *sc.sweep_map(D, sel))
            x, _ = sc.refined_solve(Am, bm)
            xe = mp.lu_solve(mp.matrix(Am.tolist()), mp.matrix(bm.tolist()))
            xs = [mp.mpf(int(np.floor(np.ldexp(m, 64)))) * mp.mpf(2) ** (int(e) - 64) for m, e in (np.frexp(v) for v in x)]  # exact
            err = max(abs(a - e) for a, e in zip(xs, xe)) / max(abs(e) for e in xe)
            assert err <= 1e-17, (D, sel, float(err))
