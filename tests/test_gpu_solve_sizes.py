"""The reduced camera system on the device (K4: csrc/mvba_solve.h, the mapped gathers of csrc/mvba_map.h, the inverse of
csrc/mvba_cov.h) at every order D at which its blocking changes (tests/_solve_cases.py), held to the backward error of the
exact system it was given: debug_read("A_full") / "b_full" are the packed [A | b] the solve started from, a parameter map
selects (or sums) D of its rows and columns, and the residual b' - A' x is formed in np.longdouble.  Every bound is LAPACK's
own figure on that same system (Cholesky: scipy cho_solve; rescue: np.linalg.solve; inverse: dpotrf + dpotri) times MARGIN,
with 2^-53 as the floor of a figure that can be exactly 0; the premises are tests/test_solve_cases_cpu.py's.  Each test prints
one row per case and collects every failing case before it asserts."""
import contextlib
import functools
import os

import numpy as np
import pytest

import _solve_cases as sc
from _solve_cases import EPS, MARGIN
from lib import _mvba
from lib.bundle_adjustment import parameter_map

pytestmark = pytest.mark.gpu

# The knobs are read by mvba_create.  MVBA_TRAIL64_MIN=0: k_chol_trail64 after every full super-block that has rows below
# it, down to one ragged 64 x 64 workgroup (nt64 = 1) -- the code path of the last updates of a large system (D = 2693:
# 40 x 64 + 6 rows).  Its bounds at nt64 = 1, read in the kernel: every row index is clamped to D (the right-hand-side row,
# which exists), every column index of C to D - 1, the k range is the finished super-block's 128 columns (the host launches
# it only for jE - jS = 128), row stride and jS are multiples of 4 (the 32-byte loads), and the stores are guarded by
# rr <= D, cc < D, cc <= rr.  Nothing in it needs a minimum size, so this mode runs the whole sweep.
MODES = {"default": {}, "launches": {"MVBA_CHOL": "launches"}, "trail64": {"MVBA_TRAIL64_MIN": "0"},
         "trail32": {"MVBA_TRAIL64_MIN": "100000000"}}


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(prob, mode="default"):
    n, m, pt_ptr, cam, xy, axis, state = prob
    with _env(MODES[mode]):
        eng = _mvba.HipEngine(n, m, pt_ptr, cam, xy, 1.0, axis)
    eng.set_params(*state)
    return eng


# ---------------------------------------------------------------- references, computed once per system
_REF = {}


def _reference(key, kind, A, b):
    """LAPACK's solution of (A, b) -- kind "chol" or "lu" --, the refined one, and LAPACK's two figures.  Cached by case; a
    cached entry is used only for the very same bits."""
    hit = _REF.get((key, kind))
    if hit is not None and np.array_equal(hit["A"], A) and np.array_equal(hit["b"], b):
        return hit
    x_ref, _ = sc.refined_solve(A, b)
    x_lap = sc.lapack_cholesky_solve(A, b) if kind == "chol" else sc.lapack_lu_solve(A, b)
    ref = {"A": A, "b": b, "x_ref": x_ref, "x_lap": x_lap, "omega": sc.omega(A, b, x_lap), "dist": sc.distance(x_lap, x_ref)}
    for v in (A, b, x_ref, x_lap):
        v.setflags(write=False)
    _REF[(key, kind)] = ref
    return ref


def _solve_case(eng, key, col, n_free, c, kind, rows, fails, set_map=True):
    """One trial under one map: the row of the table, the failures, and (x, the unit of the distance bound)."""
    if set_map:
        eng.set_parameter_map(col, n_free)
        assert eng.n_free == n_free
    eng.try_step(c)
    dxi = eng.debug_read("dxi")
    A, b = sc.mapped_system(eng.debug_read("A_full"), eng.debug_read("b_full"), col, n_free)
    x = dxi[sc.first_slots(col, n_free)]
    ref = _reference(key, kind, A, b)
    om, dist = sc.omega(A, b, x), sc.distance(x, ref["x_ref"])
    unit = max(ref["dist"], EPS * np.abs(x).max())
    U = sc.leading_untied(col, n_free)
    rows.append((key, n_free, U, om, ref["omega"], dist, ref["dist"]))
    print(f"{str(key):28s} c {c:g} D {n_free:3d} U {U:3d}  omega {om:.2e} (LAPACK {ref['omega']:.2e})  "
          f"|x - refined| {dist:.2e} (LAPACK {ref['dist']:.2e})")
    if not om <= MARGIN * max(ref["omega"], EPS):
        fails.append((key, c, "omega", om, ref["omega"]))
    if not dist <= MARGIN * unit:
        fails.append((key, c, "distance", dist, ref["dist"]))
    if not (dxi[col < 0] == 0).all():
        fails.append((key, c, "held slots moved"))
    for j in np.nonzero(np.bincount(col[col >= 0], minlength=n_free) > 1)[0]:
        if len(set(dxi[col == j].tolist())) != 1:
            fails.append((key, c, "tied slots differ", int(j)))
    return x, unit, dxi


def _summary(what, rows):
    r = np.array([row[3:] for row in rows])
    ratio = r[:, 0] / np.maximum(r[:, 1], EPS)
    print(f"{what}: {len(rows)} cases, largest omega device {r[:, 0].max():.2e}, LAPACK {r[:, 1].max():.2e}, largest ratio "
          f"{ratio.max():.2f}; largest |x - refined| device {r[:, 2].max():.2e}, LAPACK {r[:, 3].max():.2e}")


def _counts(eng):
    return eng.stats()["counts"]


def _sweep_maps():
    return [(("sweep", D, sel), *sc.sweep_map(D, sel)) for D in sc.SWEEP_D for sel in sc.SELECTIONS]


@functools.lru_cache(maxsize=None)
def _cholesky_sweep(mode):
    """The 44-camera engine in one mode, one linearisation, every D and both selections at c = 1e-4."""
    eng = _engine(sc.problem44(), mode)
    eng.linearize()
    rows, fails, xs = [], [], {}
    for key, col, n_free in _sweep_maps():
        xs[key] = _solve_case(eng, key, col, n_free, 1e-4, "chol", rows, fails)[:2]
    counts = _counts(eng)
    eng.close()
    return rows, fails, xs, counts


def _agreement(xs, base, fails, c=1e-4):
    """A mode against the default one: within the distance bound of the case."""
    for key, (x, unit) in xs.items():
        d = sc.distance(x, base[key][0])
        if not d <= MARGIN * unit:
            fails.append((key, c, "distance to the default mode", d, unit))


# ---------------------------------------------------------------- 1: the Cholesky modes over the sweep
@pytest.mark.parametrize("mode", list(MODES))
def test_cholesky_over_the_sweep(mode):
    rows, fails, xs, counts = _cholesky_sweep(mode)
    fails = list(fails)
    _summary(f"Cholesky, mode {mode}", rows)
    assert {r[1] for r in rows} == set(sc.SWEEP_D)
    if mode != "default":
        _agreement(xs, _cholesky_sweep("default")[2], fails)
    assert not fails, fails
    assert counts["lu_fallback"] == 0 and counts["barrier_fallback"] == 0


# ---------------------------------------------------------------- 2: the LU rescue over the sweep
def _rescue(eng, cases, rows, fails, set_map=True):
    for key, col, n_free in cases:
        before = _counts(eng)["lu_fallback"]
        _solve_case(eng, key, col, n_free, -1.5, "lu", rows, fails, set_map=set_map)
        if _counts(eng)["lu_fallback"] != before + 1:
            fails.append((key, -1.5, "lu_fallback did not rise by one"))


def test_lu_rescue_over_the_sweep():
    eng = _engine(sc.problem44())
    eng.linearize()
    rows, fails = [], []
    _rescue(eng, _sweep_maps(), rows, fails)
    _summary("LU rescue", rows)
    n_lu = _counts(eng)["lu_fallback"]
    assert n_lu == len(rows) == 2 * len(sc.SWEEP_D)
    # the Cholesky path is untouched afterwards
    rows2 = []
    _solve_case(eng, ("sweep", 129, "prefix"), *sc.sweep_map(129, "prefix"), 1e-4, "chol", rows2, fails)
    assert not fails, fails
    assert _counts(eng)["lu_fallback"] == n_lu and _counts(eng)["barrier_fallback"] == 0


# ---------------------------------------------------------------- 3: engines without a map (k_compact's path)
@pytest.mark.parametrize("m", list(sc.UNMAPPED))
def test_unmapped_engines_on_an_edge(m):
    prob = sc.unmapped_problem(m)
    col, n_free = parameter_map(m, prob[5])
    assert n_free == sc.UNMAPPED[m]
    key = ("unmapped", m)
    rows, fails, xs = [], [], {}
    for mode in ("default", "launches"):
        eng = _engine(prob, mode)
        assert eng.n_free == n_free
        eng.linearize()
        xs[mode] = _solve_case(eng, key, col, n_free, 1e-4, "chol", rows, fails, set_map=False)[:2]
        assert _counts(eng)["lu_fallback"] == 0 and _counts(eng)["barrier_fallback"] == 0
        if mode == "default":
            _rescue(eng, [(key, col, n_free)], rows, fails, set_map=False)
            _solve_case(eng, key, col, n_free, 1e-4, "chol", rows, fails, set_map=False)
            assert _counts(eng)["lu_fallback"] == 1
        eng.close()
    _agreement({key: xs["launches"]}, {key: xs["default"]}, fails)
    _summary(f"no map, m = {m}", rows)
    assert not fails, fails


# ---------------------------------------------------------------- 4: a tied unknown at every position; share maps
def test_tied_unknown_at_every_position_and_share_maps():
    eng = _engine(sc.problem44())
    eng.linearize()
    cases = [(("u", U), *sc.u_map(U)) for U in sc.U_SWEEP] + [(("share", s), *sc.share_map(s)) for s in sc.SHARE_SIZES]
    rows, fails = [], []
    for key, col, n_free in cases:
        _, _, dxi = _solve_case(eng, key, col, n_free, 1e-4, "chol", rows, fails)
        eng.try_step(1e-4)
        if not np.array_equal(eng.debug_read("dxi"), dxi):
            fails.append((key, 1e-4, "a second trial under the same map differs"))
    _summary("tied unknown at U, share maps", rows)
    assert [r[2] for r in rows[:len(sc.U_SWEEP)]] == list(sc.U_SWEEP)
    assert _counts(eng)["lu_fallback"] == 0 and _counts(eng)["barrier_fallback"] == 0
    rows_lu = []
    _rescue(eng, [c for c in cases if c[0] in (("u", 0), ("u", 64), ("u", 199), ("share", 44))], rows_lu, fails)
    _summary("tied unknown at U, share map of 44: LU rescue", rows_lu)
    assert len(rows_lu) == 4
    assert not fails, fails


# ---------------------------------------------------------------- 5: the inverse
INVERSE = [("prefix", D) for D in sc.INVERSE_D] + [("unmapped", m) for m in sc.INVERSE_M]


@pytest.mark.parametrize("kind,size", INVERSE, ids=[f"{k}-{s}" for k, s in INVERSE])
def test_inverse(kind, size):
    if kind == "prefix":
        prob = sc.problem44()
        col, n_free = sc.sweep_map(size, "prefix")
    else:
        prob = sc.unmapped_problem(size)
        col, n_free = parameter_map(size, prob[5])
    m = prob[1]
    eng = _engine(prob)
    if kind == "prefix":
        eng.set_parameter_map(col, n_free)
    Cf = eng.covariance(points=False, full=True)["cameras_full"]
    # mvba_covariance leaves the undamped packed system in [A | b]; cameras_full = 2 P (P^T S P)^-1 P^T
    S, _ = sc.mapped_system(eng.debug_read("A_full"), np.zeros(9 * m), col, n_free)
    eng.close()
    first = sc.first_slots(col, n_free)
    Sig = 0.5 * Cf[np.ix_(first, first)]  # (exact)
    om, om_lap = sc.omega_inverse(S, Sig), sc.omega_inverse(S, sc.lapack_potri(S))
    print(f"inverse {kind} {size}: D {n_free}  omega {om:.2e} (dpotri {om_lap:.2e}, ratio {om / max(om_lap, EPS):.2f})")
    assert om <= MARGIN * max(om_lap, EPS)
    free = np.nonzero(col >= 0)[0]
    want = np.zeros_like(Cf)
    want[np.ix_(free, free)] = Cf[np.ix_(first, first)][np.ix_(col[free], col[free])]
    assert np.array_equal(Cf, want)  # P Sigma' P^T, entry for entry: held rows and columns exactly 0
    assert np.array_equal(Cf, Cf.T)
    held = np.nonzero(col < 0)[0]
    assert (Cf[held] == 0).all() and (Cf[:, held] == 0).all()
