"""Cases shared by test_solve_cases_cpu.py and test_gpu_solve_sizes.py: the reduced camera system (K4, csrc/mvba_solve.h, with
the gathers of csrc/mvba_map.h and the inverse of csrc/mvba_cov.h) at every order D at which its blocking changes -- the
32-column tiles, the 64-row workgroups, the 128-column super-blocks, the 256-column blocks of the right-hand-side row -- set on
one 44-camera engine by hold-only parameter maps, a few engines without a map whose own D = 9 m - 7 lands on an edge, and maps
with a tied unknown at every position U of the ordering.  The reference helpers hold a solution to the backward error of the
very system the device was given (debug_read("A_full") / "b_full"), residuals in np.longdouble (omega) or exact (the
refinement); the bounds of the GPU tests are LAPACK's figures on the same systems times MARGIN.  Test infrastructure only."""
import functools
import math

import numpy as np
import scipy.linalg as sla

from _init_cases import MARGIN  # noqa: F401  (the project's factor between a measured reference figure and the bound set from it)
from lib.bundle_adjustment import gauge_slots, parameter_map
from lib.synthetic import make_scene
from oracle import ba_oracle as O

SCENE = (1500, 44, 0.3)  # 9 m - 7 = 389: three full super-blocks and a ragged fourth
M44 = SCENE[1]
D44 = 9 * M44 - 7
SWEEP_D = (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 191, 192, 193, 255, 256, 257, 319, 320, 321, 383, 384, 385, 388)
SELECTIONS = ("prefix", "scatter")
UNMAPPED = {8: 65, 15: 128, 22: 191, 29: 254, 44: 389}  # m -> D of make_scene(600, m, vis_p=0.5): k_compact's path
U_SWEEP = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 199)  # position of the tied unknown among D' = 200
U_FREE, U_TIED_CAMERAS = 201, (25, 40)  # slots left free by the held prefix; the two cameras whose f is one unknown
SHARE_SIZES = (2, 8, 9, 44)  # cameras in the one group that shares its intrinsics: nblk of k_map_tied = 1, 1, 2, 6
INVERSE_D = (1, 32, 33, 128, 129, 192, 257, 385)
INVERSE_M = (15, 22)
EPS = 2.0 ** -53  # unit roundoff of float64


# ---------------------------------------------------------------- scenes
def _state(X, K, R, t, axis):
    """tests/test_gpu_constraints.py::_state: the gauge frame, one camera body (tied parameters start equal)."""
    Xg, Rg, tg = O.normalize_scene(X, R, t, axis)
    Km = np.array(K, float)
    Km[:] = Km.mean(axis=0)
    return Xg, Km[:, 0, 0].copy(), Km[:, :2, 2].copy(), tg, Rg


@functools.lru_cache(maxsize=None)
def problem(n, m, p):
    """(n, m, pt_ptr, cam_idx, xy, axis, state) of make_scene(n, m, vis_p=p)."""
    sc = make_scene(n, m, vis_p=p)
    return n, m, sc.pt_ptr, sc.cam_idx, sc.xy, sc.axis, _state(sc.init_X, sc.init_K, sc.init_R, sc.init_t, sc.axis)


def problem44():
    return problem(*SCENE)


def unmapped_problem(m):
    return problem(600, m, 0.5)


@functools.lru_cache(maxsize=None)
def oracle_linearized(n, m, p):
    n, m, pt_ptr, cam, xy, axis, state = problem(n, m, p)
    g = O.OracleEngine(n, m, pt_ptr, cam, xy, 1.0, axis)
    g.set_params(*state)
    g.linearize()
    return g


# ---------------------------------------------------------------- maps: name -> (col, n_free)
def free_slots(m, axis):
    """The 9 m - 7 slots the gauge leaves, ascending."""
    return np.setdiff1d(np.arange(9 * m), gauge_slots(axis))


def _hold_all_but(m, axis, free):
    mask = np.ones(9 * m, bool)
    mask[free] = False
    return parameter_map(m, axis, hold=mask.reshape(m, 9))


def sweep_map(D, selection, m=M44, axis=None):
    """Hold-only: D of the non-gauge slots free -- the first D ("prefix") or a seeded random D of them ("scatter")."""
    axis = problem44()[5] if axis is None else axis
    slots = free_slots(m, axis)
    if selection == "prefix":
        free = slots[:D]
    else:
        # (seed D + 1: 73 of the 389 slots have a positive diagonal at c = -1.5, and a selection of one or two of them would
        # not reach the LU rescue -- seeds D and D + 1000 pick such a slot at D = 1; test_solve_cases_cpu.py checks every one)
        free = np.sort(np.random.default_rng(D + 1).choice(slots, size=D, replace=False))
    return _hold_all_but(m, axis, free)


def u_map(U, m=M44, axis=None):
    """D' = 200: the last 201 non-gauge slots free, f of cameras 25 and 40 one unknown, at position U of the ordering; the 199
    untied unknowns by ascending slot around it.  (Written by hand: parameter_map puts tied unknowns last.)"""
    axis = problem44()[5] if axis is None else axis
    free = free_slots(m, axis)[-U_FREE:]
    tied = np.array([9 * k for k in U_TIED_CAMERAS])
    assert np.isin(tied, free).all()
    col = np.full(9 * m, -1, np.int32)
    untied = np.setdiff1d(free, tied)
    col[untied] = np.arange(len(untied)) + (np.arange(len(untied)) >= U)
    col[tied] = U
    return col, len(untied) + 1


def share_map(size, m=M44, axis=None):
    """Cameras 0 .. size - 1 share f, u, v (three tied unknowns of `size` slots each, last in the ordering); the others keep
    their own."""
    axis = problem44()[5] if axis is None else axis
    labels = np.arange(m)
    labels[:size] = 0
    return parameter_map(m, axis, share="intrinsics", share_groups=labels)


def leading_untied(col, n_free):
    """U of mvba_set_parameter_map: the number of leading unknowns with exactly one slot."""
    cnt = np.bincount(col[col >= 0], minlength=n_free)
    U = 0
    while U < n_free and cnt[U] == 1:
        U += 1
    return U


def first_slots(col, n_free):
    """One slot per unknown (its lowest): x = dxi[first_slots]."""
    first = np.full(n_free, -1)
    for g in np.nonzero(col >= 0)[0][::-1]:
        first[col[g]] = g
    assert (first >= 0).all()
    return first


def all_maps_44():
    """Every map the GPU tests set on the 44-camera engine: key -> (col, n_free, intended n_free, intended U)."""
    out = {}
    for D in SWEEP_D + (D44,):
        for sel in SELECTIONS:
            out[("sweep", D, sel)] = sweep_map(D, sel) + (D, D)
    for U in U_SWEEP:
        out[("u", U)] = u_map(U) + (U_FREE - 1, U)
    for size in SHARE_SIZES:
        out[("share", size)] = share_map(size) + (D44 - 3 * (size - 1), D44 - 3 * size)
    return out


# ---------------------------------------------------------------- reference helpers (plain NumPy; extended precision for residuals only)
def symmetric(A_full):
    """The matrix the solve kernels read out of the packed strips: the upper triangle, mirrored (packed_sym)."""
    A = np.asarray(A_full)
    n = int(round(np.sqrt(A.size)))
    A = A.reshape(n, n)
    return np.triu(A) + np.triu(A, 1).T


def mapped_system(A_full, b_full, col, n_free):
    """(P^T A P, P^T b) with P[g][col g] = 1.  Without tied slots this is a selection: exact."""
    col = np.asarray(col)
    g = np.nonzero(col >= 0)[0]
    A, b = symmetric(A_full), np.asarray(b_full, np.float64)
    if len(g) == n_free:
        s = first_slots(col, n_free)
        return np.ascontiguousarray(A[np.ix_(s, s)]), b[s].copy()
    P = np.zeros((col.size, int(n_free)))
    P[g, col[g]] = 1.0
    return P.T @ A @ P, P.T @ b


def omega(A, b, x):
    """Componentwise backward error max_i |b - A x|_i / (|A| |x| + |b|)_i (Oettli-Prager), every product in np.longdouble."""
    Al, bl, xl = (np.asarray(v, np.longdouble) for v in (A, b, x))
    r = np.abs(bl - Al @ xl)
    den = np.abs(Al) @ np.abs(xl) + np.abs(bl)
    ok = den > 0
    assert (r[~ok] == 0).all()
    return float((r[ok] / den[ok]).max()) if ok.any() else 0.0


def refined_solve(A, b, max_iter=20):
    """(x, last): an LU solve in float64 and iterative refinement -- the running x in np.longdouble, the corrections from the
    float64 factors -- until a correction changes nothing at 2^-53 relative; last = max|correction| / max|x| of the final one.
    The residuals are exact_residual's: a residual formed in np.longdouble is good to 2^-64 |A| |x| only, and with cond up to
    3e7 the corrections then settle at 1e-16 .. 4e-15 of max|x| instead of falling (measured on these systems; at D = 31 that
    reference stood 1.3e-16 from a 40-digit solve).  AssertionError if max_iter corrections do not get there."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    lu = sla.lu_factor(A)
    x = sla.lu_solve(lu, b).astype(np.longdouble)
    for _ in range(max_iter):
        d = sla.lu_solve(lu, exact_residual(A, b, x))
        x = x + d.astype(np.longdouble)
        last = float(np.abs(d).max() / max(float(np.abs(x).max()), 1e-300))
        if last <= EPS:
            return x, last
    raise AssertionError(f"refined_solve: no convergence, last correction {last:.3e}")


def _two_prod(a, b):
    """a b = p + e exactly, elementwise in float64 (Veltkamp's split, Dekker's product; magnitudes here are far from overflow)."""
    p = a * b
    ta, tb = 134217729.0 * a, 134217729.0 * b  # 2^27 + 1
    ah, bh = ta - (ta - a), tb - (tb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def exact_residual(A, b, x):
    """b - A x for float64 A and b and np.longdouble x, every component rounded ONCE: x = xh + xl in two float64 (exact: 64
    bits in 53 + 53), A xh as error-free products, and math.fsum over b_i and the 3 n pieces of a row.  (A xl is a plain
    product: its rounding is 2^-106 |A| |x|.)"""
    x = np.asarray(x, np.longdouble)
    xh = x.astype(np.float64)
    xl = (x - xh.astype(np.longdouble)).astype(np.float64)
    p, e = _two_prod(A, xh[None, :])
    terms = np.concatenate([b[:, None], -p, -e, -(A * xl[None, :])], axis=1)
    return np.array([math.fsum(row) for row in terms.tolist()])


def distance(x, ref):
    """max|x - ref| in np.longdouble."""
    return float(np.abs(np.asarray(x, np.longdouble) - np.asarray(ref, np.longdouble)).max())


def omega_inverse(A, X):
    """The same quotient for A X - I: max_ij |A X - I|_ij / (|A| |X| + I)_ij."""
    Al, Xl = np.asarray(A, np.longdouble), np.asarray(X, np.longdouble)
    eye = np.eye(Al.shape[0], dtype=np.longdouble)
    return float((np.abs(Al @ Xl - eye) / (np.abs(Al) @ np.abs(Xl) + eye)).max())


def lapack_cholesky_solve(A, b):
    return sla.cho_solve(sla.cho_factor(A, lower=True), b)


def lapack_lu_solve(A, b):
    return np.linalg.solve(A, b)


def lapack_potri(A):
    """The inverse by dpotrf + dpotri (trtri + lauum, as k_cov_trtri / k_cov_lauum), both triangles."""
    c, info = sla.lapack.dpotrf(A, lower=1)
    assert info == 0
    inv, info = sla.lapack.dpotri(c, lower=1)
    assert info == 0
    return np.tril(inv) + np.tril(inv, -1).T
