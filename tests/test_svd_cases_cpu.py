"""The premises of tests/_svd_cases.py, proved on the host: every case's matrix has the spectrum it was built with and a
well-conditioned rank-r product, so that a miss of test_gpu_svd_forms.py cannot be blamed on the input; and the cases between
them reach every form of the Gram route that a call can reach (the routing rules are _svd_cases.py's restatement of run())."""
import re

import numpy as np
import pytest

import _svd_cases as SC

IDS = [SC.case_id(c) for c in SC.CASES]


def test_case_ids_are_unique_and_the_families_have_the_sizes_the_issue_sets():
    assert len(set(IDS)) == len(IDS)
    sizes = {f: sum(c.family == f for c in SC.CASES) for f in "abcdefg"}
    # a: 64 orders x 2; b: 16 even orders x 2 + the switch (2 row counts x 2 orders x 2); c: 10 x 2 x 2;
    # d: 2 dtypes x 4 orders x (6 uncentred + 4 centred); e: the table's 11, two float32 cases and a rank-deficient one more; f: 4; g: 2 x 5
    assert sizes == {"a": 128, "b": 40, "c": 40, "d": 80, "e": 14, "f": 4, "g": 10}
    assert max(c.rows * c.n for c in SC.CASES) <= 5000 * 64


@pytest.mark.parametrize("c", SC.CASES, ids=IDS)
def test_premises(c):
    """k = min(rows, n); LAPACK returns the constructed spectrum to 1e-10 (uncentred cases, on the float64 matrix before any
    cast); sigma_{r+1} / sigma_r <= 0.5 on LAPACK's values of the data the device sees, centred and float32 cases included."""
    k, r = min(c.rows, c.n), c.rank
    s = SC.constructed(c)
    assert len(s) == (4 if c.graded else k) and 1 <= r <= k
    Wt = SC.matrix(c)
    assert Wt.shape == (c.rows, c.n) and Wt.dtype == np.dtype(c.dtype) and Wt.flags.c_contiguous
    if not c.center:
        s_lapack = np.linalg.svd(SC.known_spectrum(c.rows, c.n, s), compute_uv=False)
        err = np.abs(s_lapack[:len(s)] - s).max()
        print(f"constructed spectrum against LAPACK: {err:.3e} (<= 1e-10)")
        assert err <= 1e-10 and np.all(s_lapack[len(s):] <= 1e-10)
    ref = SC.reference(c)
    assert ref.sigma.shape == (c.n,) and ref.product.shape == (c.n, c.rows) and np.all(ref.sigma[k:] == 0.0)
    if r < c.n:
        ratio = ref.sigma[r] / ref.sigma[r - 1]
        print(f"sigma_{r + 1} / sigma_{r} = {ratio:.4f} (<= 0.5)")
        assert ratio <= 0.5
    if c.center:
        assert np.abs(ref.mean - SC.OFFSET).max() < 1.0  # |mean| >> spread: G - s s^T / N would cancel


def test_every_reachable_form_is_reached():
    reached = set()
    for c in SC.CASES:
        cells = SC.cells(c)
        assert cells <= SC.TABLE, sorted(cells - SC.TABLE)
        reached |= cells
    assert set(SC.UNREACHABLE) <= SC.TABLE and all(SC.UNREACHABLE.values())
    assert not reached & set(SC.UNREACHABLE), sorted(reached & set(SC.UNREACHABLE))
    empty = SC.TABLE - reached - set(SC.UNREACHABLE)
    assert not empty, sorted(empty)


def test_the_cells_the_issue_names_are_reached_by_the_cases_it_names():
    """The holes of the issue, one by one, each pinned to the family meant to close it."""
    def reach(family, pattern):
        return [c for c in SC.CASES if c.family == family and any(re.search(pattern, x) for x in SC.cells(c))]

    assert {c.n for c in reach("a", r"k_gram_pair<double> 4 tile rows")} == set(range(49, 65))  # orders 49 .. 64
    assert [c.n for c in reach("a", r"more than 64 KiB")] == [64, 64] and SC.jacobi_lds(64) == 66336 and SC.jacobi_lds(63) <= 65536
    assert {c.n for c in reach("b", r"k_rotate_rows<double> .*, centred")} == set(range(2, 33, 2))  # every width it admits
    assert {(c.rows, c.n) for c in reach("b", r"below the streaming form's rows")} == {(4095, 24), (4095, 32)}
    assert {c.n for c in reach("b", r"one k-step")} == {2, 4}
    assert {(c.rows, c.n) for c in reach("c", r"k_gram_fused<float> partial last vector")} == {(4097, 1), (4097, 7), (4097, 23), (4097, 30)}
    assert {(c.rows, c.n) for c in reach("d", r"k_gram_fused<double> partial last vector")} >= {(4097, 7), (129, 7), (1, 7)}
    assert {c.n for c in reach("c", r"k_gram_pair<float>")} == {33, 49, 64}
    assert {c.n for c in reach("c", r"whole rows as float4")} == {16, 24, 32, 64}
    assert {c.n for c in reach("e", r"k_jacobi<false>")} == {65, 100, 128, 255, 256}
    assert {c.dtype for c in reach("e", r"chunked, centred")} == {"float32", "float64"}
    assert {c.n for c in reach("e", r"k_rotate<double> several column blocks")} == {65, 100, 255, 256}
    assert {c.n for c in reach("a", r"means switch the lean path off")} == {16, 24, 32}
    for c in SC.FAMILY_E:
        assert SC.route(c) == SC.EXPECTED_ROUTE[c], SC.case_id(c)
    # the partial double2 of the issue's family d: an odd element count
    assert all((c.rows * c.n) % 2 == 1 for c in SC.CASES if (c.rows, c.n) in ((4097, 7), (4097, 33)))


def test_the_restated_rules_at_their_edges():
    """The same edges as csrc/host_check.cpp holds wide_route and rotate_streams to."""
    assert not SC.wide_route(64, 1) and not SC.wide_route(64, 17)
    assert SC.wide_route(65, 16) and not SC.wide_route(65, 17)
    assert SC.wide_route(256, 16) and not SC.wide_route(256, 17) and SC.wide_route(257, 17)
    for n in range(1, 41):
        assert SC.rotate_streams(8, 4096, n) == (n % 2 == 0 and n <= 32)
        assert SC.rotate_streams(4, 4096, n) == (n % 4 == 0 and n <= 32)
        assert not SC.rotate_streams(8, 4095, n)
    assert [SC.gram_mode(n) for n in (1, 16, 17, 24, 25, 32, 33)] == [1, 1, 2, 2, 3, 3, 0]
    assert SC.gram_pairs(33) == 6 and SC.gram_pairs(49) == 10 and SC.gram_pairs(64) == 10 and SC.gram_pairs(256) == 136 and SC.gram_pairs(24) == 2
