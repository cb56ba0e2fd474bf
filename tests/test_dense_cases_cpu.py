"""The cases of tests/_dense_cases.py reach what they are named for -- every tile count of k_schur_dense, both chunk sizes and
role splits, every remainder of N modulo the chunk, 65 workgroups, workgroups of 3 | 2 and 7 | 6 chunks, points of mixed sign
codes on well-conditioned blocks -- shown on the host from the restated launch rule, the text of csrc/mvba_dense.h and the oracle
alone; and the host-versus-host figures that the GPU bounds at SIGN_C are MARGIN x of are re-measured here."""
import os
import re

import numpy as np
import pytest

import _dense_cases as D

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d-reconstruction-from-multi-view-exp_amd", "csrc")
SQUARED = [c for m in D.SWEEP for c in D.sweep_cases(m) if c.loss == "squared"]


def _id(case):
    return f"{case.n}x{case.m}x{case.vis:g}"


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _rule(text, name):
    """`constexpr int name(int T) { return T <op> K ? A : B; }` of the header as a function of T."""
    mt = re.search(r"constexpr int %s\(int T\) \{ return T (==|<=) (\d+) \? (\d+) : (\d+); \}" % name, text)
    assert mt, name
    op, k, a, b = mt.group(1), int(mt.group(2)), int(mt.group(3)), int(mt.group(4))
    return lambda T: a if (T == k if op == "==" else T <= k) else b


# ---------------------------------------------------------------- the launch rule
def test_launch_restates_the_header():
    """dense_ch, dense_wgs, dense_consumers, DENSE_MAX_TILES and the prefetch depth read from the text of csrc/mvba_dense.h, the
    tile count and the workgroup count from csrc/mvba_create.h: a changed rule fails here instead of silently emptying a GPU test."""
    dense, create, device = _text("mvba_dense.h"), _text("mvba_create.h"), _text("mvba_device.h")
    max_tiles = int(re.search(r"constexpr int DENSE_MAX_TILES = (\d+);", dense).group(1))
    assert max_tiles == D.tiles(D.MAX_CAMERAS) == 12 and D.tiles(D.MAX_CAMERAS + 1) > max_tiles
    ch, wgs, nc = _rule(dense, "dense_ch"), _rule(dense, "dense_wgs"), _rule(dense, "dense_consumers")
    rec = int(re.search(r"constexpr int REC = (\d+);", device).group(1))
    assert "constexpr int MMAX = (16 * T) / 9;" in dense and "NPRE = (MMAX * REC + 63) / 64" in dense
    for T in range(1, max_tiles + 1):
        assert (D.chunk_points(T), D.workgroups_per_cu(T), D.consumers(T)) == (ch(T), wgs(T), nc(T)), T
        assert D.npre(T) == ((16 * T) // 9 * rec + 63) // 64
    assert "const int T = (9 * m + 15) / 16;" in create
    assert ("h->dense_blocks = (int)std::max<long long>(1, std::min<long long>((N + dense_ch(T) - 1) / dense_ch(T), "
            "(long long)n_cu_dense * dense_wgs(T)));") in create
    assert "hipDeviceGetAttribute(&n_cu_dense, hipDeviceAttributeMultiprocessorCount, h->device);" in create
    for n, m, n_cu in ((1, 2, 256), (54, 21, 256), (259, 8, 256), (13297, 14, 256), (13305, 6, 304)):
        T, CH, W, n_chunks = D.launch(n, m, n_cu)
        assert (T, CH, n_chunks) == ((9 * m + 15) // 16, ch(T), -(-n // ch(T))) and W == max(1, min(n_chunks, n_cu * wgs(T)))
    assert D.launch(54, 21, 256) == (12, 4, 14, 14) and D.launch(13297, 14, 256) == (8, 8, 256, 1663)


def test_sweep_covers_every_camera_count_tile_count_and_remainder():
    assert list(D.SWEEP) == list(range(2, 22))
    assert {D.tiles(m) for m in D.SWEEP} == set(range(2, 13))  # (T = 1 would be one camera: mvba_create refuses it)
    assert {D.chunk_points(D.tiles(m)) for m in D.SWEEP} == {4, 8} and {D.consumers(D.tiles(m)) for m in D.SWEEP} == {4, 8}
    assert {D.npre(D.tiles(m)) for m in D.SWEEP} == {1, 2, 3}
    for CH in (4, 8):
        rem = {n % CH for m, sizes in D.SWEEP.items() if D.chunk_points(D.tiles(m)) == CH for n in sizes}
        assert rem == set(range(CH)), (CH, rem)
    # every tile count of the eight-consumer split and of the four-consumer split sees a part-filled last chunk
    for T in range(2, 13):
        assert any(n % D.chunk_points(T) for m, sizes in D.SWEEP.items() if D.tiles(m) == T for n in sizes), T
    big = [(m, n) for m, sizes in D.SWEEP.items() for n in sizes if n > 100]
    assert big == [(8, 259), (17, 259)] and D.tiles(8) <= 8 < 9 <= D.tiles(17)
    for m, n in big:  # 65 workgroups on any device of 65 / 33 compute units or more: lane 0 of the finish kernel sums two partial tiles
        assert D.launch(n, m, 256)[2:] == (65, 65) and D.launch(n, m, 65)[2] == 65
    assert all(30 <= n <= 60 for sizes in D.SWEEP.values() for n in sizes if n < 100)
    for m in D.SWEEP:
        cases = D.sweep_cases(m)
        assert len(cases) == 4 * len(D.SWEEP[m]) and {(c.vis, c.loss) for c in cases} == set(D.SWEEP_VARIANTS)
    assert set(D.SWEEP_SIGN) == {(c.n, c.m, c.vis) for c in SQUARED}


@pytest.mark.parametrize("m", list(D.SWEEP))
def test_table_variants_miss_observations_and_stay_dense(m):
    """The table variants list at least 60 % of the (point, camera) pairs but not all, no camera twice in a point, every camera
    seen; the contiguous ones list every pair in order."""
    for case in D.sweep_cases(m):
        n, m_, pt_ptr, cam, xy = D.problem(case)[:5]
        deg = np.diff(pt_ptr)
        assert len(pt_ptr) == n + 1 and pt_ptr[-1] == len(cam) == len(xy) and set(cam.tolist()) == set(range(m))
        pt = np.repeat(np.arange(n), deg)
        assert (np.diff(cam.astype(np.int64))[pt[1:] == pt[:-1]] > 0).all()
        if case.vis >= 1.0:
            assert (deg == m).all()
        else:
            assert deg.min() >= 1 and (deg < m).any() and len(cam) >= 0.6 * n * m


def test_depth_representatives_are_one_per_depth_chunk_and_split():
    for m, (T, pre, CH, nc) in D.DEPTH.items():
        assert (D.tiles(m), D.npre(T), D.chunk_points(T), D.consumers(T)) == (T, pre, CH, nc)
    assert {v[1:] for v in D.DEPTH.values()} == {(1, 4, 4), (2, 8, 4), (2, 4, 8), (3, 4, 8)}
    assert sorted(D.DEPTH_TABLE_P.values()) == [0.65, 0.8, 0.8, 0.8]


@pytest.mark.parametrize("n_cu", [256, 304, 64])
def test_depth_cases_give_workgroups_q_and_q_minus_one_chunks(n_cu):
    for m in D.DEPTH:
        for q in D.DEPTH_Q:
            n = D.depth_points(m, q, n_cu)
            T, CH, W, n_chunks = D.launch(n, m, n_cu)
            assert W == n_cu * D.workgroups_per_cu(T) and n % CH != 0
            r = n_chunks - (q - 1) * W
            assert 0 < r < W and D.chunks_per_workgroup(n_chunks, W) == {q: r, q - 1: W - r}
            # workgroup w runs the chunks w, w + W, ...: restated by counting
            count = np.bincount(np.arange(n_chunks) % W, minlength=W)
            assert sorted(set(count.tolist())) == [q - 1, q] and (count == q).sum() == r
    assert D.depth_points(14, 7, 256) == 13297 and D.depth_points(6, 7, 256) == 13305


# ---------------------------------------------------------------- signs
@pytest.fixture(scope="module", params=SQUARED, ids=_id)
def lin(request):
    return request.param, D.oracle(request.param)


def test_sign_c_is_the_first_candidate_with_mixed_codes_on_conditioned_blocks(lin):
    """At SIGN_C: at least two different sign codes, a point whose three rows do not share a sign, every damped block conditioned
    below 1e4, an indefinite reduced matrix -- and no earlier candidate gives that."""
    case, g = lin
    c = D.SWEEP_SIGN[(case.n, case.m, case.vis)][0]
    assert c == D.pick_sign_c(g) and c in D.SIGN_CANDIDATES
    codes = D.sign_codes(g, c)
    assert len(set(codes.tolist())) >= 2 and ((codes != 0) & (codes != 7)).any()
    assert D.damped_condition(g, c) < D.COND_LIMIT == 1e4
    # the codes carry the inertia of the damped block (Sylvester: E'^-1 = L D L^T has as many negative d as E' negative eigenvalues)
    Ec = g.E.copy()
    Ec[:, np.arange(3), np.arange(3)] *= 1.0 + c
    n_neg = (np.linalg.eigvalsh(Ec) < 0).sum(axis=1)
    assert (n_neg == ((codes & 1) + ((codes >> 1) & 1) + ((codes >> 2) & 1))).all()  # (inertia)
    g.try_step(c)
    w = np.linalg.eigvalsh(g.A)
    assert w.min() < 0 < w.max()
    ref = D.reference(case)
    assert ref.sign_c == c and ref.eig_s[0] < 0 < ref.eig_s[1] and np.isfinite(ref.E1_s)


def test_the_older_negative_damping_gives_no_mixed_rows_to_speak_of(lin):
    """The gap: at c = -1.5, the damping of every older negative-damping test, at most one row of a point is positive -- codes 5, 6, 7
    only --, and with seven cameras or more and full visibility every point has code 7,
    where a bit order reversed within a point or a sign on the wrong row of an MFMA step changes nothing."""
    case, g = lin
    codes = set(D.sign_codes(g, D.ALL_NEGATIVE_C).tolist())
    assert codes <= {5, 6, 7}
    if case.m >= 7 and case.vis >= 1.0:
        assert codes == {7}


def test_recorded_host_versus_host_figures(lin):
    """The oracle's float64 reduced_system against blockdiag - F^T E'^-1 F in long double on the same linearisation, at SIGN_C:
    within a factor of 2 of the figure recorded in tests/_dense_cases.py.  The sum taken in double on (high + low) parts -- the
    way the depth cases' figures are measured -- gives the same figure wherever it matters (above 1e-14)."""
    case, g = lin
    c, rec = D.SWEEP_SIGN[(case.n, case.m, case.vis)]
    d = D.host_diff(g, c)
    print(f"{_id(case)}: SIGN_C {c}, host versus host |dA| / max|A| = {d:.3e} (recorded {rec:.1e}) -> GPU bound {D.sign_bound(rec):.1e}")
    assert 0.5 * rec <= d <= 2.0 * rec
    d2 = D.host_diff(g, c, sum_in_double=True)
    assert abs(d2 - d) <= 0.1 * d + 2e-15


def test_premises_bite():
    """A scene at the older damping fails the sign premise, and a launch rule with one workgroup per CU moves the depth sizes."""
    g = D.oracle(D.Case(48, 15, 1.0, "squared"))
    assert not D.sign_premise(g, D.ALL_NEGATIVE_C) and D.sign_premise(g, -0.8)
    n = D.depth_points(6, 7, 256)
    T, CH, W, n_chunks = D.launch(n, 6, 128)  # (half the workgroups: 13 | 12 chunks each, not 7 | 6)
    assert set(D.chunks_per_workgroup(n_chunks, W)) == {12, 13}


def test_depth_reference_measures_its_own_figure():
    """A depth-sized case (the smallest: 2 W + r chunks of 21 cameras on 64 compute units) meets the sweep's premise at its
    SIGN_C and carries the host-versus-host figure measured on it; the 14-camera sizes of a 256-CU device do not (a block
    conditioned worse than 1e4 at every candidate) and take the best-conditioned candidate with mixed signs."""
    case = D.depth_case(21, 3, False, 64)
    ref = D.reference(case)
    codes = set(D.sign_codes(D.oracle(case), ref.sign_c).tolist())
    assert len(codes) >= 2 and codes - {0, 7} and ref.eig_s[0] < 0 < ref.eig_s[1]
    assert 0 < ref.host_diff_s < 1e-10  # (MARGIN x it stays far below what a lost chunk moves A by, CH / N ~ 1e-3)
    assert D.sign_premise(D.oracle(case), ref.sign_c)
    assert D.reference(D.depth_case(21, 3, True, 64), sign=False).sign_c is None
    g = D.oracle(D.depth_case(14, 3, False, 256))
    assert not any(D.sign_premise(g, c) for c in D.SIGN_CANDIDATES)
    c = D.pick_sign_c(g, best_effort=True)
    assert D.sign_premise(g, c, np.inf) and D.damped_condition(g, c) == min(D.damped_condition(g, k) for k in D.SIGN_CANDIDATES)
    with pytest.raises(AssertionError):
        D.pick_sign_c(g)
