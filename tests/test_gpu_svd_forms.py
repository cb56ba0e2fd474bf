"""The Gram route of the thin SVD, form by form (the cases and the form each one reaches: tests/_svd_cases.py; their premises
and coverage: tests/test_svd_cases_cpu.py; the list of forms: DESIGN.md §4).  Every test builds its own workspace -- create,
load, run, close -- and compares with LAPACK in float64 on the same data (minus its float64 column means when centred), or with
the constructed spectrum for the graded cases.  The tolerances are those the suite already holds in test_gpu_factorization.py:
  fp64   every sigma rtol 1e-9 + 1e-12 sigma_1, M^T M 1e-12, M S against the rank-r truncation 1e-8 sigma_1, sweeps < 30
         (test_every_order_of_the_small_eigen_solver); means 1e-11 (test_wide_matrices_vs_lapack)
  fp32   sigma[:r] rtol 2e-6, M S 1e-5 sigma_1 (test_wide_matrices_vs_lapack); M^T M 1e-5, means 1e-5
         (test_large_tall_skinny_properties; half an ulp of float32 at the offset 40 is 1.9e-6); the rest of sigma finite
  graded sigma[:4] against the constructed values rtol 1e-7, M^T M 1e-12 (test_fp64_graded_spectrum_small_singular_values_like_gesdd)
  fewer rows than columns: the n - k singular values that are exactly zero within 10 sqrt(n eps) sigma_1, the floor of one
         fp64 Gram pass (an eigenvalue error of order n eps sigma_1^2) with a margin of 10
Every check prints what it observed next to its tolerance.

Worst observed on an MI355X (one run, 308 cases in 6 s), next to the tolerance.  sigma: the largest |error| / sigma_i over
every singular value held (fp64: all min(rows, n); fp32: the leading r); fp64 stays below the 1e-12 sigma_1 floor everywhere.
  family      sigma            M^T M - I        M S / sigma_1    means            sweeps (last pass)
  a  fp64     1.3e-13 (1e-9)   2.9e-14 (1e-12)  1.2e-14 (1e-8)   2.3e-13 (1e-11)  2  (< 30)
  b  fp64     1.7e-13 (1e-9)   1.7e-14 (1e-12)  2.0e-14 (1e-8)   2.1e-13 (1e-11)  1
  c  fp32     3.9e-8  (2e-6)   3.7e-8  (1e-5)   3.6e-9  (1e-5)   1.9e-6  (1e-5)   15
  d  fp64     3.0e-13 (1e-9)   1.9e-14 (1e-12)  2.4e-14 (1e-8)   2.5e-13 (1e-11)  12 (3 x 33; 1 x 33: 10)
  d  fp32     3.9e-8  (2e-6)   3.8e-8  (1e-5)   3.3e-8  (1e-5)   1.9e-6  (1e-5)   14
  e  fp64     1.8e-13 (1e-9)   1.0e-13 (1e-12)  7.9e-15 (1e-8)   1.1e-13 (1e-11)  21 (20 x 100)
  e  fp32     4.2e-8  (2e-6)   1.9e-8  (1e-5)   2.5e-9  (1e-5)   1.9e-6  (1e-5)   18
  f  graded   6.7e-12 (1e-7)   3.4e-14 (1e-12)
  g  fp64     5.7e-14 (1e-9)   1.6e-14 (1e-12)  8.4e-15 (1e-8)   1.5e-13 (1e-11)  2
  exactly zero singular values (d: 1, 3 rows; e: 20 x 100): at most 6.0e-15 (10 sqrt(n eps) sigma_1 = 3.2e-6 .. 1.2e-5)
The float32 means sit at half an ulp of float32 at 40 (1.9e-6): they are computed in fp64 and rounded once.
Before k_jacobi took its pivot as the mean of its two copies (csrc/mvsvd_jacobi.h), the cases with eigenvalues that are exactly
zero at 33 and more columns (d: 1 x 33 and 3 x 33 in both dtypes; e: 20 x 100) ran all 60 sweeps and failed `sweeps < 30`.
"""
import numpy as np
import pytest

import _svd_cases as SC
from lib import _mvba

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _ids(cases):
    return [SC.case_id(c) for c in cases]


class _Checks:
    """Observed figures next to their tolerances: printed one by one, asserted together at the end, so that a failing case shows
    every figure of it."""

    def __init__(self, c):
        self.c, self.failed = c, []

    def hold(self, name, observed, tol, strict=False):
        ok = bool(observed < tol) if strict else bool(observed <= tol)
        line = f"{SC.case_id(self.c)}: {name} {observed:.3e} ({'<' if strict else '<='} {tol:.3e}){'' if ok else '  MISSED'}"
        print(line)
        if not ok:
            self.failed.append(line)

    def note(self, text):
        print(f"{SC.case_id(self.c)}: {text}")

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def _factorise(c, Wt, ws=None):
    own = ws is None
    if own:
        ws = _mvba.SvdWorkspace(c.rows, c.n, np.dtype(c.dtype))
    try:
        ws.load(Wt)
        return ws.run(c.rank, center=c.center)
    finally:
        if own:
            ws.close()


def _compare(c, out, ref, block=False):
    """The case's result against its reference, with the tolerances of the module docstring."""
    M, sig, S, mu, tm = out
    r, k, n = c.rank, min(c.rows, c.n), c.n
    f32 = c.dtype == "float32"
    assert M.shape == (n, r) and S.shape == (r, c.rows) and sig.shape == (n,) and M.dtype == S.dtype == sig.dtype == np.dtype(c.dtype)
    M64, S64, sig64 = M.astype(np.float64), S.astype(np.float64), sig.astype(np.float64)
    s1 = ref.sigma[0]
    ck = _Checks(c)
    lead = r if (f32 or block) else k  # fp32 is not held on its trailing singular values; the block iteration computes 32
    d = np.abs(sig64[:lead] - ref.sigma[:lead])
    if f32:
        ck.hold(f"sigma[:{lead}] relative", (d / ref.sigma[:lead]).max(), 2e-6)
    else:  # |d| <= 1e-9 sigma_i + 1e-12 sigma_1, as assert_allclose(rtol=1e-9, atol=1e-12 sigma_1) reads it
        ck.note(f"sigma[:{lead}] plain relative error {(d / ref.sigma[:lead]).max():.3e}, absolute per sigma_1 {d.max() / s1:.3e}")
        ck.hold(f"sigma[:{lead}] relative, beyond 1e-12 sigma_1", (np.maximum(d - 1e-12 * s1, 0.0) / ref.sigma[:lead]).max(), 1e-9)
    if block:
        assert np.all(np.isfinite(sig64[:SC.WB])) and np.all(np.isnan(sig64[SC.WB:])), "the block iteration returns 32 Ritz values, NaN beyond"
    else:
        assert np.all(np.isfinite(sig64)), "every singular value of the Gram route is finite"
        if not f32 and k < n:
            ck.hold(f"sigma[{k}:] (exactly zero)", np.abs(sig64[k:]).max(), 10.0 * np.sqrt(n * EPS) * s1)
    ck.hold("M^T M - I", np.abs(M64.T @ M64 - np.eye(r)).max(), 1e-5 if f32 else 1e-12)
    ck.hold("M S - rank-r truncation, per sigma_1", np.abs(M64 @ S64 - ref.product).max() / s1, 1e-5 if f32 else 1e-8)
    if not block:
        ck.hold("sweeps", tm["sweeps"], 30, strict=True)
    if c.center:
        ck.hold("means", np.abs(mu.astype(np.float64) - ref.mean).max(), 1e-5 if f32 else 1e-11)
    else:
        assert np.all(mu == 0), "no means without centring"
    return ck, tm


def _gram_route_case(c):
    assert SC.route(c) == "gram"
    ref = SC.reference(c)
    ck, tm = _compare(c, _factorise(c, ref.Wt), ref)
    # fp64 takes the second, preconditioned pass; float32 none (run(): refine = sizeof(T) == 8)
    assert (tm["refine_ms"] > 0) == (c.dtype == "float64"), tm
    ck.done()


@pytest.mark.parametrize("c", SC.FAMILY_A, ids=_ids(SC.FAMILY_A))
def test_every_order_up_to_64_fp64(c):
    """a. Every order 1 .. 64 at 3000 rows, centred and not: k_gram_fused in its three modes, lean and general, k_gram_pair with
    three and four tile rows; k_jacobi_small (order 1, order 2, odd orders), k_jacobi<true> up to order 64, where it takes more
    than 64 KiB of LDS; k_rotate (3000 < 4096 rows); k_project's element-wise rows."""
    _gram_route_case(c)


@pytest.mark.parametrize("c", SC.FAMILY_B, ids=_ids(SC.FAMILY_B))
def test_the_streaming_rotation_at_every_width(c):
    """b. k_rotate_rows at every even order 2 .. 32, 4173 rows (odd, the last step ends inside a wave tile), centred and not; 4095
    against 4096 rows at 24 and 32 columns: the switch between the two rotation forms."""
    _gram_route_case(c)


@pytest.mark.parametrize("c", SC.FAMILY_C, ids=_ids(SC.FAMILY_C))
def test_float32_forms(c):
    """c. float32 through every Gram form, the pair form, k_project's float4 rows and element-wise rows; 4097 rows of 1, 7, 23 and
    30 columns end in a partial float4."""
    _gram_route_case(c)


@pytest.mark.parametrize("c", SC.FAMILY_D, ids=_ids(SC.FAMILY_D))
def test_row_edges(c):
    """d. One row, fewer rows than columns, one GRAM_ROWS step ended exactly and by one row, 4097 rows (an odd element count at 7
    and 33 columns: a partial double2), both dtypes."""
    _gram_route_case(c)


@pytest.mark.parametrize("c", SC.FAMILY_E, ids=_ids(SC.FAMILY_E))
def test_route_boundaries(c):
    """e. 64 | 65 columns, 16 | 17 triplets, 256 | 257 columns.  The route is pinned by what the call returns: every sigma finite
    and (fp64) refine_ms > 0 on the Gram route, sigma[32:] all NaN after the block iteration, ValueError beyond both."""
    expected = SC.EXPECTED_ROUTE[c]
    assert SC.route(c) == expected
    if expected == "refused":
        ws = _mvba.SvdWorkspace(c.rows, c.n, np.dtype(c.dtype))
        try:
            ws.load(SC.matrix(c))
            with pytest.raises(ValueError, match="n_rank <= 16"):
                ws.run(c.rank)
        finally:
            ws.close()
        return
    ref = SC.reference(c)
    ck, tm = _compare(c, _factorise(c, ref.Wt), ref, block=expected == "block")
    if expected == "gram":
        assert (tm["refine_ms"] > 0) == (c.dtype == "float64"), tm
    ck.done()


@pytest.mark.parametrize("c", SC.FAMILY_F, ids=_ids(SC.FAMILY_F))
def test_graded_spectra_through_each_rotation_form(c):
    """f. sigma_4 = 1e-7 sigma_1 through k_rotate_rows (4173 x 30) and k_rotate (3000 x 30, 33, 64): one Gram pass would leave
    sigma_4 good to 1e-2; the constructed values are the reference (exact to eps sigma_1)."""
    M, sig, S, _mu, tm = _factorise(c, SC.matrix(c))
    s = SC.constructed(c)
    ck = _Checks(c)
    ck.hold("sigma[:4] relative, against the constructed values", np.abs(sig[:4] / s - 1.0).max(), 1e-7)
    ck.hold("M^T M - I", np.abs(M.T @ M - np.eye(4)).max(), 1e-12)
    assert tm["refine_ms"] > 0 and np.all(np.isfinite(sig))
    ck.done()


@pytest.mark.parametrize("n", [24, 40])
def test_one_workspace_smaller_loads_and_centring_switched(n):
    """g. A workspace of 5000 rows loaded with 5000, 129 and 4100 rows, centring switched on and off between the runs, every run
    against LAPACK: partial tiles, column-sum slices and means of the larger run must not reach the smaller one."""
    cases = [c for c in SC.FAMILY_G if c.n == n]
    assert cases[0].rows == 5000
    ws = _mvba.SvdWorkspace(5000, n, np.float64)
    checks = []
    try:
        for c in cases:
            ref = SC.reference(c)
            ck, tm = _compare(c, _factorise(c, ref.Wt, ws), ref)
            assert tm["refine_ms"] > 0
            checks.append(ck)
    finally:
        ws.close()
    for ck in checks:
        ck.done()
