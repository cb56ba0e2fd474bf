"""The dense Schur form (k_schur_dense, csrc/mvba_dense.h) at every tile count, past the second chunk of a workgroup and on
mixed signs of E^-1 = R S R^T: the cases, the restated launch rule and the references.  Test infrastructure only.

Premises (that the cases reach what they are named for, that the reference is accurate on them): tests/test_dense_cases_cpu.py.
The kernel against the reference: tests/test_gpu_dense_form.py."""
import functools
from collections import namedtuple

import numpy as np

from _init_cases import MARGIN  # noqa: F401  (the project's factor between a measured reference error and the bound set from it)
from _robust_ref import RobustOracleEngine, inject_outliers
from lib.bundle_adjustment import to_gauge_frame
from lib.synthetic import make_scene
from oracle import ba_oracle as O

C = 1e-2                          # the ordinary trial
SIGN_CANDIDATES = (-0.8, -0.9, -0.95)
ALL_NEGATIVE_C = -1.5             # the damping of every older negative-damping test: sign codes 5, 6, 7; 7 at every point from 7 cameras on
HUBER = ("huber", 3.0)            # tests/test_gpu_robust.py: loss and scale ...
OUTLIERS = (0.08, 20.0, 100.0, 5)  # ... and its inject_outliers(frac, lo, hi, seed)
TABLE_P = 0.8
MAX_CAMERAS = 21


# ---------------------------------------------------------------- the launch rule of csrc/mvba_dense.h and csrc/mvba_create.h, restated
def tiles(m):
    return (9 * m + 15) // 16


def chunk_points(T):
    return 8 if T == 8 else 4


def workgroups_per_cu(T):
    return 2 if T <= 7 else 1


def consumers(T):
    return 4 if T <= 8 else 8


def npre(T):
    """Prefetch registers per lane and set: the 8 record slots of the instantiation's 16 T // 9 cameras over 64 lanes."""
    return ((16 * T) // 9 * 8 + 63) // 64


def launch(n_points, m, n_cu):
    """(T, CH, workgroups, n_chunks) of k_schur_dense for n_points x m on a device of n_cu compute units."""
    T = tiles(m)
    CH = chunk_points(T)
    n_chunks = (n_points + CH - 1) // CH
    return T, CH, max(1, min(n_chunks, n_cu * workgroups_per_cu(T))), n_chunks


def chunks_per_workgroup(n_chunks, W):
    """{chunks: workgroups that run so many}: workgroup w takes the chunks w, w + W, ..."""
    q, r = divmod(n_chunks, W)
    return {k: v for k, v in ((q + 1, r), (q, W - r)) if v and k}


# ---------------------------------------------------------------- cases
# vis: 1.0 = every point lists every camera (one contiguous range of records), else through the (point, camera) table
Case = namedtuple("Case", "n m vis loss")


def _sweep_sizes(m):
    """The point counts of camera count m: a few dozen, every remainder modulo the chunk size over the sweep -- the 4-point
    chunks over consecutive camera counts, the 8-point chunks (13 and 14 cameras only) with four sizes each --, and at 8 and
    17 cameras 65 CH - 1 points: 65 workgroups, the first count at which a lane of k_schur_dense_finish sums two partial tiles."""
    CH = chunk_points(tiles(m))
    if CH == 8:
        return tuple(40 + 4 * (m - 13) + i for i in range(4))  # 40 .. 43 and 44 .. 47: the remainders 0 .. 7
    return (33 + m,) + ((65 * CH - 1,) if m in (8, 17) else ())


SWEEP = {m: _sweep_sizes(m) for m in range(2, MAX_CAMERAS + 1)}
SWEEP_VARIANTS = [(1.0, "squared"), (TABLE_P, "squared"), (1.0, "huber"), (TABLE_P, "huber")]


def sweep_cases(m):
    return [Case(n, m, vis, loss) for n in SWEEP[m] for vis, loss in SWEEP_VARIANTS]


# m: (T, NPRE, CH, consumers) -- one representative per (prefetch depth, chunk size, role split)
DEPTH = {6: (4, 1, 4, 4), 14: (8, 2, 8, 4), 15: (9, 2, 4, 8), 21: (12, 3, 4, 8)}
DEPTH_TABLE_P = {6: 0.8, 14: 0.8, 15: 0.8, 21: 0.65}
DEPTH_Q = (3, 7)  # the chunks of the busier workgroups: n_chunks = (q - 1) W + r


def depth_points(m, q, n_cu):
    """N for which the W workgroups of m cameras on n_cu compute units run q chunks (r = W // 2 - 1 of them) or q - 1, with N no
    multiple of the chunk size: q = 3 leaves the producer loop at its first exit with one set re-fetched, q = 7 runs both halves in
    steady state with every set re-fetched inside the loop and leaves at the first exit again; the q - 1 = 6 of the other
    workgroups leave at the second."""
    T = tiles(m)
    CH, W = chunk_points(T), n_cu * workgroups_per_cu(T)
    r = W // 2 - 1
    assert 0 < r < W, "a device of at least two compute units"
    n = ((q - 1) * W + r) * CH - (1 if q == 3 else CH - 1)  # three live points in the last chunk (CH = 4) / one
    assert n % CH != 0
    return n


def depth_case(m, q, table, n_cu):
    return Case(depth_points(m, q, n_cu), m, DEPTH_TABLE_P[m] if table else 1.0, "squared")


# ---------------------------------------------------------------- problems and references
@functools.lru_cache(maxsize=4)
def _scene(n, m, vis):
    """make_scene's observation list; where its repair of points below three views leaves no missing observation (2 and 3 cameras),
    the full scene with the last observation of every third point taken out."""
    if vis >= 1.0 or m > 3:
        sc = make_scene(n, m, vis_p=vis, project="numpy")
        return sc, sc.pt_ptr, sc.cam_idx, sc.xy
    sc = make_scene(n, m, vis_p=1.0, project="numpy")
    keep = np.ones((n, m), bool)
    keep[::3, m - 1] = False
    keep = keep.reshape(-1)
    pt_ptr = np.concatenate([[0], np.cumsum(keep.reshape(n, m).sum(1))]).astype(np.int64)
    return sc, pt_ptr, sc.cam_idx[keep], sc.xy[keep]


def problem(case):
    """(n, m, pt_ptr, cam, xy, f0, axis, X, f, u, t, R): the arguments of an engine and its state in the gauge frame."""
    sc, pt_ptr, cam, xy = _scene(case.n, case.m, case.vis)
    if case.loss != "squared":
        xy = inject_outliers(xy, *OUTLIERS[:3], seed=OUTLIERS[3])[0]
    X, R, t = to_gauge_frame(sc.init_X, sc.init_R, sc.init_t, sc.axis)
    return (case.n, case.m, pt_ptr, cam, xy, 1.0, sc.axis, X, sc.init_K[:, 0, 0], sc.init_K[:, :2, 2], t, R)


def engine_kwargs(case):
    return {} if case.loss == "squared" else {"loss": case.loss, "loss_scale": HUBER[1]}


def oracle(case):
    """The oracle on the case, linearised at its state."""
    n, m, pt_ptr, cam, xy, f0, axis, *state = problem(case)
    g = (O.OracleEngine if case.loss == "squared" else RobustOracleEngine)(n, m, pt_ptr, cam, xy, f0, axis, **engine_kwargs(case))
    g.set_params(*state)
    g.linearize()
    return g


def sign_codes(g, c):
    """The sign code of every point at damping c as k_point_inv forms it: L D L^T of the inverse of the damped E_a without
    pivoting, 1 (d0 < 0) + 2 (d1 < 0) + 4 (d2 < 0).  (The kernel stores the code + 1.)"""
    Ec = g.E.copy()
    i3 = np.arange(3)
    Ec[:, i3, i3] *= 1.0 + c
    I = np.linalg.inv(Ec)
    d0 = I[:, 0, 0]
    l10, l20 = I[:, 0, 1] / d0, I[:, 0, 2] / d0
    d1 = I[:, 1, 1] - l10 * I[:, 0, 1]
    l21 = (I[:, 1, 2] - l20 * I[:, 0, 1]) / d1
    d2 = I[:, 2, 2] - l20 * I[:, 0, 2] - l21 * l21 * d1
    return (d0 < 0) * 1 + (d1 < 0) * 2 + (d2 < 0) * 4


def damped_condition(g, c):
    """The worst condition number of a damped 3 x 3 block."""
    Ec = g.E.copy()
    i3 = np.arange(3)
    Ec[:, i3, i3] *= 1.0 + c
    return float(np.linalg.cond(Ec).max())


COND_LIMIT = 1e4  # of a damped block at SIGN_C: what keeps the float64 reference itself accurate


def sign_premise(g, c, cond_limit=COND_LIMIT):
    """At least two different codes, a point whose three rows do not share a sign, blocks conditioned below the limit."""
    codes = set(sign_codes(g, c).tolist())
    return len(codes) >= 2 and bool(codes - {0, 7}) and damped_condition(g, c) < cond_limit


def pick_sign_c(g, best_effort=False):
    """The first candidate damping at which g meets the premise.  ``best_effort`` (the depth cases: among thousands of points of
    14 cameras some damped block is conditioned worse than COND_LIMIT at every candidate): failing that, the candidate with mixed
    signs whose worst block is conditioned best -- the host-versus-host figure measured with the reference says what it costs."""
    for c in SIGN_CANDIDATES:
        if sign_premise(g, c):
            return c
    mixed = [c for c in SIGN_CANDIDATES if best_effort and sign_premise(g, c, np.inf)]
    if mixed:
        return min(mixed, key=lambda c: damped_condition(g, c))
    raise AssertionError("no candidate damping gives this case mixed signs on well-conditioned blocks")


def reduced_matrix_longdouble(g, c, sum_in_double=False):
    """blockdiag(G_k + c diag G_k) - F^T E'^-1 F in np.longdouble on the float64 linearisation of g (E'^-1 by cofactors).
    ``sum_in_double``: E'^-1 and E'^-1 F in long double -- where an ill-conditioned block costs the oracle its digits --, the
    sum over the points in float64 on (high + low) parts of E'^-1 F: rounding of ~sqrt(3 N) 1e-16 of max|A| instead of seconds
    of long-double products at thousands of points; for figures far above that only (the depth cases)."""
    L = np.longdouble
    E, F, G = g.E.astype(L), g.F.astype(L), g.G.astype(L)
    i3 = np.arange(3)
    E[:, i3, i3] *= L(1) + L(c)
    a, b, cc, d, e, f = E[:, 0, 0], E[:, 0, 1], E[:, 0, 2], E[:, 1, 1], E[:, 1, 2], E[:, 2, 2]
    c00, c01, c02 = d * f - e * e, cc * e - b * f, b * e - cc * d
    det = a * c00 + b * c01 + cc * c02
    inv = np.empty_like(E)
    inv[:, 0, 0], inv[:, 0, 1], inv[:, 0, 2] = c00 / det, c01 / det, c02 / det
    inv[:, 1, 1], inv[:, 1, 2], inv[:, 2, 2] = (a * f - cc * cc) / det, (b * cc - a * e) / det, (a * d - b * b) / det
    inv[:, 1, 0], inv[:, 2, 0], inv[:, 2, 1] = inv[:, 0, 1], inv[:, 0, 2], inv[:, 1, 2]
    Y = (inv[g.pt][:, :, :, None] * F[:, None, :, :]).sum(axis=2)  # E'^-1 F_ak (n_obs, 3, 9)
    m = g.m
    cols = 9 * g.cam[:, None] + np.arange(9)

    def rows(V, dtype):  # (n_obs, 3, 9) -> (3 N, 9 m): the three rows of every point over all camera columns
        out = np.zeros((g.n, 3, 9 * m), dtype)
        for r in range(3):
            out[g.pt[:, None], r, cols] = V[:, r, :]
        return out.reshape(-1, 9 * m)

    if sum_in_double:
        Yh = Y.astype(np.float64)
        Fw = rows(g.F, np.float64)
        A = -((Fw.T @ rows(Yh, np.float64)).astype(L) + (Fw.T @ rows((Y - Yh).astype(np.float64), np.float64)).astype(L))
    else:
        A = -(rows(F, L).T @ rows(Y, L))
    for k in range(m):
        Gk = G[k].copy()
        Gk[np.arange(9), np.arange(9)] *= L(1) + L(c)
        A[9 * k:9 * k + 9, 9 * k:9 * k + 9] += Gk
    return A


def host_diff(g, c, A=None, sum_in_double=False):
    """max |A_float64 - A_longdouble| / max|A|: the oracle's own error in A at damping c."""
    A = g.reduced_system(c)[0] if A is None else A
    Al = reduced_matrix_longdouble(g, c, sum_in_double)
    return float(np.abs(A.astype(np.longdouble) - Al).max() / np.abs(Al).max())


# The host-versus-host figure for A at SIGN_C of every squared sweep case, keyed (points, cameras, visibility) -> (SIGN_C, figure):
# measured and re-checked by tests/test_dense_cases_cpu.py.  A GPU assert on A at SIGN_C gets MARGIN x the figure with the ordinary
# bound on A, 1e-11 max|A|, as its floor.  (A depth case's size follows the device: its figure is measured with its reference.)
SWEEP_SIGN = {
    (35, 2, 1.0): (-0.8, 5.0e-16), (35, 2, 0.8): (-0.8, 4.3e-16),
    (36, 3, 1.0): (-0.8, 1.7e-14), (36, 3, 0.8): (-0.8, 1.5e-14),
    (37, 4, 1.0): (-0.8, 5.0e-16), (37, 4, 0.8): (-0.8, 4.3e-16),
    (38, 5, 1.0): (-0.8, 4.2e-16), (38, 5, 0.8): (-0.8, 1.3e-15),
    (39, 6, 1.0): (-0.8, 3.0e-15), (39, 6, 0.8): (-0.8, 4.3e-15),
    (40, 7, 1.0): (-0.8, 7.0e-16), (40, 7, 0.8): (-0.8, 3.5e-15),
    (41, 8, 1.0): (-0.8, 1.7e-13), (41, 8, 0.8): (-0.8, 1.9e-13), (259, 8, 1.0): (-0.8, 4.7e-13), (259, 8, 0.8): (-0.8, 4.8e-13),
    (42, 9, 1.0): (-0.8, 6.0e-16), (42, 9, 0.8): (-0.8, 1.5e-15),
    (43, 10, 1.0): (-0.9, 2.1e-14), (43, 10, 0.8): (-0.8, 1.9e-15),
    (44, 11, 1.0): (-0.8, 9.2e-16), (44, 11, 0.8): (-0.8, 2.6e-15),
    (45, 12, 1.0): (-0.9, 9.0e-16), (45, 12, 0.8): (-0.8, 8.1e-16),
    (40, 13, 1.0): (-0.8, 1.3e-15), (40, 13, 0.8): (-0.8, 1.1e-15), (41, 13, 1.0): (-0.8, 1.2e-15), (41, 13, 0.8): (-0.8, 1.0e-15),
    (42, 13, 1.0): (-0.8, 1.2e-15), (42, 13, 0.8): (-0.8, 1.0e-15), (43, 13, 1.0): (-0.8, 1.3e-15), (43, 13, 0.8): (-0.8, 1.0e-15),
    (44, 14, 1.0): (-0.8, 6.0e-14), (44, 14, 0.8): (-0.8, 4.4e-15), (45, 14, 1.0): (-0.8, 6.7e-14), (45, 14, 0.8): (-0.8, 4.3e-15),
    (46, 14, 1.0): (-0.8, 7.1e-14), (46, 14, 0.8): (-0.8, 4.4e-15), (47, 14, 1.0): (-0.8, 7.1e-14), (47, 14, 0.8): (-0.8, 4.3e-15),
    (48, 15, 1.0): (-0.8, 3.2e-16), (48, 15, 0.8): (-0.8, 2.5e-16),
    (49, 16, 1.0): (-0.9, 5.6e-16), (49, 16, 0.8): (-0.8, 2.1e-14),
    (50, 17, 1.0): (-0.8, 7.0e-16), (50, 17, 0.8): (-0.8, 1.8e-14), (259, 17, 1.0): (-0.8, 1.4e-14), (259, 17, 0.8): (-0.8, 3.3e-14),
    (51, 18, 1.0): (-0.8, 3.0e-15), (51, 18, 0.8): (-0.8, 2.7e-15),
    (52, 19, 1.0): (-0.8, 1.6e-14), (52, 19, 0.8): (-0.8, 3.8e-15),
    (53, 20, 1.0): (-0.8, 3.3e-14), (53, 20, 0.8): (-0.8, 3.0e-14),
    (54, 21, 1.0): (-0.8, 1.0e-15), (54, 21, 0.8): (-0.8, 1.9e-15),
}


def sign_bound(figure):
    """The bound on |dA| / max|A| at SIGN_C from the case's host-versus-host figure."""
    return max(1e-11, MARGIN * figure)


Reference = namedtuple("Reference", "A b E1 sign_c A_s b_s E1_s dxi_s eig_s host_diff_s")


@functools.lru_cache(maxsize=None)
def reference(case, sign=True):
    """The oracle's reduced system and trial cost at C and -- squared loss, ``sign`` -- at the case's SIGN_C: the system, the
    trial cost, the increment of that trial (full length, zeros at the gauge slots), the extreme eigenvalues of the gauge-free
    matrix and the host-versus-host figure (recorded: a sweep case; measured here with the sum in double: a depth case, whose
    SIGN_C is pick_sign_c's best effort).  Computed once per case, read-only."""
    g = oracle(case)
    A, b = g.reduced_system(C)
    E1 = g.try_step(C)
    out = [A, b, E1] + [None] * 7
    if case.loss == "squared" and sign:
        key = (case.n, case.m, case.vis)
        if key in SWEEP_SIGN:
            c, figure = SWEEP_SIGN[key]
        else:
            c, figure = pick_sign_c(g, best_effort=True), None
        A_s, b_s = g.reduced_system(c)
        if figure is None:
            figure = host_diff(g, c, A_s, sum_in_double=True)
        E1_s = g.try_step(c)
        dxi = np.zeros(9 * case.m)
        dxi[g.keep] = g.dxi_red
        w = np.linalg.eigvalsh(g.A)
        out[3:] = [c, A_s, b_s, E1_s, dxi, (float(w.min()), float(w.max())), figure]
    for v in out:
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return Reference(*out)
