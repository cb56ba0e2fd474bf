"""Cases for the Gram route of the thin SVD (csrc/mvsvd_gram.h, mvsvd_jacobi.h, mvsvd_rows.h; run() and create_workspace()
in csrc/mvsvd.hip), in the style of tests/_degree_cases.py: test_svd_cases_cpu.py proves their premises and their coverage on
the host, test_gpu_svd_forms.py runs them.  Test infrastructure only.

One construction for every case, a matrix with a known spectrum (`matrix`): W = U diag(s) V^T with U, V from seeded QR,
k = min(rows, n), r = min(n_rank, k), s = linspace(8, 4, r) | logspace(0, -3, k - r).  sigma_{r+1} / sigma_r is 0.25 by
construction, so the rank-r product is well conditioned at every shape.  Centred cases add 40 to every entry; float32 cases cast
the matrix, and their reference is LAPACK in float64 on the cast data.  The graded cases are s = GRADED, rank 4, no noise.

The routing rules of run() are restated here in Python (`route`), to be read against wide_route, rotate_streams, gram_mode,
gram_tiles, jacobi_kernel / jacobi_lds and project_lds in csrc/mvba_host.h and csrc/mvsvd.hip and against the kernels' own
branches (lean, the partial-vector tail, k_project's three load forms).  `cells(case)` names every form a case runs; TABLE is
every form there is, UNREACHABLE the instantiations no call can reach."""
import collections
import functools

import numpy as np

# ---------------------------------------------------------------- the sizes of csrc/mvba_host.h
GT, GRAM_ROWS, WIDE_MIN, JACOBI_MAX, WB, JW, JACOBI_LDS_ORDER, PC = 16, 128, 64, 256, 32, 32, 64, 64
ROTATE_ROWS_MIN = 4096  # rotate_streams
GRADED = (1.0, 0.3, 1e-3, 1e-7)
OFFSET = 40.0  # what a centred case adds to every entry (as test_wide_matrices_vs_lapack)

Case = collections.namedtuple("Case", "family rows n dtype rank center graded")


def case_id(c):
    return f"{c.family}-{c.rows}x{c.n}-{'f32' if c.dtype == 'float32' else 'f64'}-r{c.rank}{'-centred' if c.center else ''}{'-graded' if c.graded else ''}"


def _c(family, rows, n, dtype="float64", rank=3, center=False, graded=False):
    return Case(family, rows, n, dtype, min(rank, n, rows), bool(center), bool(graded))


# ---------------------------------------------------------------- the cases, family by family
BOTH = (False, True)
# a. every order of the Gram route up to WIDE_MIN, fp64, below the streaming rotation's row count: k_rotate
FAMILY_A = [_c("a", 3000, n, center=ce) for n in range(1, 65) for ce in BOTH]
# b. k_rotate_rows at every width it admits, the last step ending inside a wave tile (4173 = 32 * 128 + 77), and its switch
FAMILY_B = ([_c("b", 4173, n, center=ce) for n in range(2, 33, 2) for ce in BOTH]
            + [_c("b", rows, n, center=ce) for rows in (4095, 4096) for n in (24, 32) for ce in BOTH])
# c. float32: every Gram form, the pair form, k_project's float4 and element-wise rows; 4097 x 7 / 23 / 30 end in a partial float4
FAMILY_C = [_c("c", rows, n, "float32", center=ce) for n in (1, 7, 16, 23, 24, 30, 32, 33, 49, 64) for rows in (3000, 4097) for ce in BOTH]
# d. row edges: one row, fewer rows than columns, one GRAM_ROWS step ended exactly and by one row, an odd element count
FAMILY_D = [_c("d", rows, n, dt, center=ce) for dt in ("float64", "float32") for n in (7, 24, 32, 33) for rows in (1, 3, 127, 128, 129, 4097)
            for ce in BOTH if rows >= 127 or not ce]
# e. the route boundaries: (columns, rank, rows, dtype, centred, expected route)
BOUNDARIES = [
    (64, 16, 3000, "float64", False, "gram"),
    (64, 17, 3000, "float64", False, "gram"),  # five projection groups, the last of one vector
    (65, 16, 1000, "float64", False, "block"),
    (65, 17, 1000, "float64", False, "gram"),  # k_jacobi<false> at an odd order
    (100, 17, 1000, "float32", False, "gram"),  # chunked projection in float
    (100, 17, 1000, "float32", True, "gram"),  # (beyond the issue's list: the float pair form and chunked projection with means)
    (100, 17, 1000, "float64", True, "gram"),  # chunked smu
    (128, 17, 1000, "float32", False, "gram"),  # (beyond the issue's list: two full projection chunks in float)
    (100, 17, 20, "float64", False, "gram"),  # (beyond the issue's list: k_jacobi<false> on 80 eigenvalues that are exactly zero)
    (255, 17, 1000, "float64", False, "gram"),
    (256, 17, 1000, "float64", False, "gram"),  # 16 tile rows, 136 pairs, four full chunks, four column blocks of k_rotate
    (256, 17, 1000, "float64", True, "gram"),
    (256, 16, 1000, "float64", False, "block"),
    (257, 17, 1000, "float64", False, "refused"),
]
FAMILY_E = [_c("e", rows, n, dt, rank=r, center=ce) for n, r, rows, dt, ce, _route in BOUNDARIES]
EXPECTED_ROUTE = {_c("e", rows, n, dt, rank=r, center=ce): rt for n, r, rows, dt, ce, rt in BOUNDARIES}
# f. graded spectra through each rotation form
FAMILY_F = [_c("f", rows, n, rank=4, graded=True) for rows, n in ((4173, 30), (3000, 30), (3000, 33), (3000, 64))]
# g. one workspace of 5000 rows, loaded with 5000, 129 and 4100 rows, centring switched between the runs
REUSE_ROWS = ((5000, False), (129, True), (4100, False), (4100, True), (129, False))
FAMILY_G = [_c("g", rows, n, center=ce) for n in (24, 40) for rows, ce in REUSE_ROWS]

CASES = FAMILY_A + FAMILY_B + FAMILY_C + FAMILY_D + FAMILY_E + FAMILY_F + FAMILY_G


# ---------------------------------------------------------------- the construction
def spectrum(rows, n, n_rank):
    k = min(rows, n)
    r = min(n_rank, k)
    return np.concatenate([np.linspace(8.0, 4.0, r) if r > 1 else np.full(r, 8.0), np.logspace(0.0, -3.0, k - r)])


def known_spectrum(rows, n, s):
    """_graded's recipe (tests/test_gpu_factorization.py): U diag(s) V^T, U (rows, len(s)) and V (n, len(s)) from seeded QR."""
    rng = np.random.default_rng(1000 * n + rows)
    U, _ = np.linalg.qr(rng.normal(size=(rows, len(s))))
    V, _ = np.linalg.qr(rng.normal(size=(n, len(s))))
    return (U * np.asarray(s)) @ V.T


@functools.lru_cache(maxsize=None)
def constructed(c):
    """The singular values the case's matrix is built from (before the offset of a centred case and the cast of a float32 one)."""
    s = np.array(GRADED) if c.graded else spectrum(c.rows, c.n, c.rank)
    s.setflags(write=False)
    return s


def matrix(c):
    """The (rows, n) array the workspace is loaded with, in the case's dtype."""
    W = known_spectrum(c.rows, c.n, constructed(c))
    if c.center:
        W = W + OFFSET
    return np.ascontiguousarray(W.astype(c.dtype))


Reference = collections.namedtuple("Reference", "Wt mean sigma product")


def reference(c):
    """LAPACK in float64 on the data the device sees (minus its float64 column means when centred): the float64 column means,
    every singular value (n of them: zeros beyond min(rows, n)), the rank-r truncation (n, rows)."""
    Wt = matrix(c)
    W64 = Wt.astype(np.float64)
    mean = W64.mean(axis=0)
    if c.center:
        W64 = W64 - mean
    U, s, Vt = np.linalg.svd(W64.T, full_matrices=False)
    r = c.rank
    sigma = np.zeros(c.n)
    sigma[:len(s)] = s
    return Reference(Wt, mean, sigma, (U[:, :r] * s[:r]) @ Vt[:r])


# ---------------------------------------------------------------- the routing rules of run(), restated
def el(dtype):
    return 4 if dtype == "float32" else 8


def wide_route(n, n_rank):  # mvba_host.h: wide_route, with create_workspace's wide = n > WIDE_MIN
    return n > WIDE_MIN and (n_rank <= WB // 2 or n > JACOBI_MAX)


def rotate_streams(elb, rows, n):  # mvba_host.h: rotate_streams
    return n <= 32 and n % 2 == 0 and (n * elb) % 16 == 0 and rows >= ROTATE_ROWS_MIN


def gram_mode(n):
    return 1 if n <= 16 else (2 if n <= 24 else (3 if n <= 32 else 0))


def gram_tiles(n):
    return (n + GT - 1) // GT


def gram_pairs(n):
    return 2 if gram_mode(n) == 2 else gram_tiles(n) * (gram_tiles(n) + 1) // 2


def jacobi_lds(n):
    half = ((n + 1) & ~1) // 2
    return 0 if n <= JW else 8 * (3 * half + 2) + 16 + (16 * n * n if n <= JACOBI_LDS_ORDER else 0)


def route(c):
    if not wide_route(c.n, c.rank):
        return "gram"
    return "block" if c.rank <= WB // 2 else "refused"


def _tiles_class(n):
    t = gram_tiles(n)
    return "3 tile rows" if t == 3 else ("4 tile rows" if t == 4 else "5 .. 16 tile rows")


def _gram_cells(T, rows, n, centred):
    """One Gram pass over a (rows, n) matrix of type T."""
    mode, out = gram_mode(n), set()
    how = "centred" if centred else "uncentred"
    if mode:
        lean_width = {1: 16, 2: 24, 3: 32}[mode]
        if n == lean_width:
            operand = "lean width, means switch the lean path off" if centred else "lean"
        else:
            operand = "general, centred" if centred else "general"
        out.add(f"k_gram_fused<{T}, {mode}> {operand}")
        vec = 16 // (4 if T == "float" else 8)
        out.add(f"k_gram_fused<{T}> {'partial last vector' if (rows * n) % vec else 'whole vectors'}")
        out.add(f"k_gram_fused {'one step' if rows <= GRAM_ROWS else 'several steps'}, {'ends on a step' if rows % GRAM_ROWS == 0 else 'ends inside a step'}")  # (the row loop is the same text for both types)
    else:
        out.add(f"k_gram_pair<{T}> {_tiles_class(n)}, {how}")
        out.add(f"k_gram_pair<{T}> {'last tile full' if n % GT == 0 else 'last tile part-filled'}")
    return out


def cells(c):
    """Every form of the Gram route that the case runs (empty for a case that takes the block iteration or is refused)."""
    if route(c) != "gram":
        return {f"route: {route(c)}"}
    T = "float" if c.dtype == "float32" else "double"
    n, rows, out = c.n, c.rows, {"route: gram"}
    refine = el(c.dtype) == 8  # run(): refine = sizeof(T) == 8
    out |= _gram_cells(T, rows, n, c.center)
    # the eigen-solver (jacobi_kernel), twice with a second pass
    if n <= JW:
        out.add("k_jacobi_small " + ("order 1" if n == 1 else ("order 2, one pair" if n == 2 else ("odd order" if n % 2 else "even order"))))
    elif n <= JACOBI_LDS_ORDER:
        out.add("k_jacobi<true> " + ("odd order" if n % 2 else "even order"))
        if jacobi_lds(n) > 64 * 1024:
            out.add("k_jacobi<true> more than 64 KiB of LDS")
    else:
        out.add("k_jacobi<false> " + ("odd order" if n % 2 else "even order"))
    out.add("second pass" if refine else "one pass (float32)")
    if refine:
        how = "centred" if c.center else "uncentred"
        if rotate_streams(el(c.dtype), rows, n):
            nct, ng = (n + 15) // 16, (n + 3) // 4
            tiles = "one column tile, all lanes live" if n == 16 else ("one column tile" if nct == 1 else ("two column tiles, both full" if n == 32 else "two column tiles"))
            out.add(f"k_rotate_rows<double> {tiles}, {how}")
            if ng == 1:
                out.add("k_rotate_rows<double> one k-step")
            out.add(f"k_rotate_rows<double> {'partial last vector' if (rows * n) % 2 else 'whole vectors'}")
            out.add(f"k_rotate_rows<double> {'ends on a step' if rows % GRAM_ROWS == 0 else 'ends inside a step'}")
        else:
            blocks = (n + 63) // 64
            out.add(f"k_rotate<double> {'one column block' if blocks == 1 else 'several column blocks'}, {how}")
            if n <= 32 and n % 2 == 0:
                out.add("k_rotate<double> below the streaming form's rows")
        out |= _gram_cells("double", rows, n, False)  # the Gram matrix of B = (W - mu) V1: fp64, never centred
    # the projection, in groups of four basis vectors
    how = "centred" if c.center else "uncentred"
    if n > PC:
        out.add(f"k_project<{T}> chunked, {how}")
        out.add(f"k_project<{T}> chunked, {'last chunk full' if n % PC == 0 else 'last chunk part-filled'}")
    elif T == "float" and n % 4 == 0:
        out.add(f"k_project<float> whole rows as float4, {how}")
    else:
        out.add(f"k_project<{T}> whole rows element-wise, {how}")
    out.add(f"k_project<{T}> {'one group' if c.rank <= 4 else 'several groups'}")
    out.add(f"k_project<{T}> {'fewer than 64 rows' if rows < 64 else ('last wave tile part-filled' if rows % 64 else 'last wave tile full')}")
    return out


def _table():
    t = {"route: gram", "route: block", "route: refused", "second pass", "one pass (float32)"}
    for T in ("float", "double"):
        for mode in (1, 2, 3):
            for operand in ("lean", "lean width, means switch the lean path off", "general", "general, centred"):
                t.add(f"k_gram_fused<{T}, {mode}> {operand}")
        for x in ("partial last vector", "whole vectors"):
            t.add(f"k_gram_fused<{T}> {x}")
        for steps in ("one step", "several steps"):
            for end in ("ends on a step", "ends inside a step"):
                t.add(f"k_gram_fused {steps}, {end}")
        for tiles in ("3 tile rows", "4 tile rows", "5 .. 16 tile rows"):
            for how in ("centred", "uncentred"):
                t.add(f"k_gram_pair<{T}> {tiles}, {how}")
        for x in ("last tile full", "last tile part-filled"):
            t.add(f"k_gram_pair<{T}> {x}")
        for how in ("centred", "uncentred"):
            t.add(f"k_project<{T}> chunked, {how}")
            t.add(f"k_project<{T}> whole rows element-wise, {how}")
            t.add(f"k_project<{T}> whole rows as float4, {how}")
            t.add(f"k_rotate<{T}> one column block, {how}")
            t.add(f"k_rotate<{T}> several column blocks, {how}")
            for tiles in ("one column tile, all lanes live", "one column tile", "two column tiles, both full", "two column tiles"):
                t.add(f"k_rotate_rows<{T}> {tiles}, {how}")
        for x in ("chunked, last chunk full", "chunked, last chunk part-filled", "one group", "several groups", "fewer than 64 rows", "last wave tile part-filled", "last wave tile full"):
            t.add(f"k_project<{T}> {x}")
        for x in ("one k-step", "partial last vector", "whole vectors", "ends on a step", "ends inside a step"):
            t.add(f"k_rotate_rows<{T}> {x}")
        t.add(f"k_rotate<{T}> below the streaming form's rows")
    for x in ("order 1", "order 2, one pair", "odd order", "even order"):
        t.add(f"k_jacobi_small {x}")
    for x in ("odd order", "even order"):
        t.add(f"k_jacobi<true> {x}")
        t.add(f"k_jacobi<false> {x}")
    t.add("k_jacobi<true> more than 64 KiB of LDS")
    return t


TABLE = _table()


def _unreachable():
    u = {}
    for cell in TABLE:
        if cell.startswith(("k_rotate<float>", "k_rotate_rows<float>")):
            u[cell] = "float32 data takes no second pass (run(): refine = sizeof(T) == 8)"
        elif cell == "k_rotate_rows<double> partial last vector":
            u[cell] = "the streaming form takes an even number of fp64 columns (rotate_streams): rows * n is even, every 16-byte vector whole"
        elif cell.startswith("k_project<double> whole rows as float4"):
            u[cell] = "the float4 rows of k_project are taken for 4-byte elements only"
    return u


UNREACHABLE = _unreachable()
