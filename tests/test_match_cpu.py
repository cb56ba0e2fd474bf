"""Descriptor matching, the parts that need no GPU: the NumPy reference against an independent formulation on
every case, the premises of the GPU cases, the exported symbol with its argument errors and its empty calls, the input forms of
match_descriptors, and the premise of the end-to-end GPU test."""
import ctypes
import os

import numpy as np
import pytest

from lib import _mvba
from lib.initialization import descriptor_arrays, match_descriptors

import _match_cases as MC
import _match_ref as MR


def _independent(A, B, ratio, mutual, max_dist2):
    """(best, best2, second2, code) of one directed pair from float64 differences (exact: every term is an integer below 2^53) and
    a stable argsort per query -- no expansion into norms and dot products, no argmin."""
    na, nb = len(A), len(B)
    D = np.zeros((na, nb))
    if na <= nb:
        for a in range(na):
            diff = B.astype(np.float64) - A[a].astype(np.float64)
            D[a] = (diff * diff).sum(axis=1)
    else:  # (the same differences, a candidate at a time: the loop stays short with 10^5 queries of 5 candidates)
        for b in range(nb):
            diff = A.astype(np.float64) - B[b].astype(np.float64)
            D[:, b] = (diff * diff).sum(axis=1)
    order = np.argsort(D, axis=1, kind="stable")  # by (distance, index)
    rows = np.arange(na)
    best = order[:, 0] if nb else np.full(na, -1)
    best2 = D[rows, best] if nb else np.full(na, -1.0)
    second2 = D[rows, order[:, 1]] if nb > 1 else np.full(na, -1.0)
    if nb == 0:
        return best, best2, second2, np.full(na, MR.NO_CANDIDATE)
    back = np.argsort(D.T, axis=1, kind="stable")[:, 0] if na else np.zeros(nb, np.int64)
    far = (best2 > max_dist2) if max_dist2 >= 0 else np.zeros(na, bool)
    amb = np.zeros(na, bool) if ratio is None else ((second2 < 0) | ~(best2 < np.float64(ratio) * np.float64(ratio) * second2))
    lone = (back[best] != rows) if mutual else np.zeros(na, bool)
    code = np.where(far, MR.FAR, np.where(amb, MR.AMBIGUOUS, np.where(lone, MR.NOT_MUTUAL, MR.KEPT)))
    return best, best2, second2, code


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_reference_against_an_independent_formulation(name):
    _reference_against_independent(MC.case(name), MC.reference(name))


@pytest.mark.parametrize("name", sorted(MC.LIMIT_CASES))
def test_limit_reference_against_an_independent_formulation(name):
    _reference_against_independent(MC.limit_case(name), MC.limit_reference(name))


def _reference_against_independent(case, ref):
    kp_ptr, desc, pairs, kw = case
    at = 0
    for i, (k, l) in enumerate(pairs):
        A, B = desc[kp_ptr[k]:kp_ptr[k + 1]], desc[kp_ptr[l]:kp_ptr[l + 1]]
        best, best2, second2, code = _independent(A, B, kw["ratio"], kw["mutual"], kw["max_dist2"])
        sl = slice(at, at + len(A))
        np.testing.assert_array_equal(ref["nn_best"][sl], best)
        np.testing.assert_array_equal(ref["nn_dist2"][sl], best2)
        np.testing.assert_array_equal(ref["nn_second2"][sl], second2)
        np.testing.assert_array_equal(ref["code"][sl], code)
        keep = np.nonzero(code == MR.KEPT)[0]
        m = slice(ref["match_ptr"][i], ref["match_ptr"][i + 1])
        np.testing.assert_array_equal(ref["kp_pairs"][m], np.stack([keep, best[keep]], axis=1))
        np.testing.assert_array_equal(ref["dist2"][m], best2[keep])
        at += len(A)
    assert at == ref["n_queries"] == len(ref["code"]) and ref["n_matches"] == ref["match_ptr"][-1] == len(ref["kp_pairs"])
    assert sum(ref[k] for k in MR.COUNTS if k != "n_queries") == ref["n_queries"]


def test_premises_of_the_cases():
    kp_ptr, desc, pairs, _ = MC.case("tiles")
    sizes = {(int(kp_ptr[k + 1] - kp_ptr[k]), int(kp_ptr[l + 1] - kp_ptr[l])) for k, l in pairs}
    assert sizes == {(a, b) for a in MC.N_K for b in MC.N_L} and len(pairs) == 45
    assert MC.N_K == (1, 127, 128, 129, 259) and MC.N_L == (1, 2, 31, 32, 33, 127, 128, 129, 261) and MC.KSTEP == 32
    r = MC.reference("tiles")
    assert r["n_matches"] > 0 and r["n_ambiguous"] > 0 and r["n_not_mutual"] > 0
    for d in MC.DIMS:
        assert MC.case(f"dim{d}")[1].shape == (115, d)
    assert 16 % MC.KSTEP and 48 % MC.KSTEP and 496 % MC.KSTEP  # the zero padding of a k step
    r = MC.reference("flat")  # every distance the largest there is: every tie to index 0, the second equals the best
    assert (r["nn_dist2"] == MC.FLAT_D2).all() and (r["nn_second2"] == MC.FLAT_D2).all() and (r["nn_best"] == 0).all()
    assert r["kp_pairs"].tolist() == [[0, 0], [0, 0]] and r["match_ptr"].tolist() == [0, 1, 2]  # mutual: query 0 and candidate 0 alone
    r = MC.reference("flat_one")
    assert (r["nn_best"][:40] == 17).all() and (r["nn_dist2"][:40] == MC.FLAT_D2 - 255 ** 2 + 254 ** 2).all() and (r["nn_second2"][:40] == MC.FLAT_D2).all()
    r, perm = MC.reference("orientation"), MC.orientation_perm()
    np.testing.assert_array_equal(r["nn_best"], perm)
    np.testing.assert_array_equal(r["nn_dist2"], (np.arange(MC.ORIENT_N) + 1) ** 2)
    kp_ptr, desc, _, _ = MC.case("orientation")
    D = MR.distance2(desc[:MC.ORIENT_N], desc[MC.ORIENT_N:])
    assert (np.argmin(D.T[:MC.ORIENT_N], axis=1) != perm).mean() > 0.9  # rows and columns swapped: another answer
    r = MC.reference("dup_candidates")  # the smaller index of the two, the second equals the best, ambiguous at ratio 1
    assert (r["nn_best"] == 2 * np.arange(30)).all() and (r["nn_second2"] == r["nn_dist2"]).all() and r["n_ambiguous"] == 30 and r["n_matches"] == 0
    r = MC.reference("dup_queries")  # the mutual check keeps the smaller index
    assert r["kp_pairs"].tolist() == [[2 * i, i] for i in range(30)] and r["n_not_mutual"] == 30
    r = MC.reference("rules")
    assert min(r["n_matches"], r["n_no_candidate"], r["n_far"], r["n_ambiguous"], r["n_not_mutual"]) >= 1
    kp_ptr, _, pairs, _ = MC.case("rules")
    counts = np.diff(kp_ptr).tolist()
    assert counts == [40, 30, 0, 1] and pairs.tolist() == [[0, 1], [2, 1], [0, 2], [0, 3], [1, 0], [3, 0]]
    assert r["match_ptr"][2] == r["match_ptr"][1] == r["match_ptr"][3]  # no query, then no candidate
    assert r["match_ptr"][4] == r["match_ptr"][3] and r["n_no_candidate"] == 40  # a single candidate passes no ratio test
    at = 40 + 0 + 40
    assert (r["nn_second2"][at:at + 40] == -1).all() and (r["code"][at:at + 40] != MR.KEPT).all()
    assert MC.reference("rules_no_ratio")["n_ambiguous"] == 0
    p = MC.reference("rules_plain")  # no ratio, no distance test: the single candidate takes the one query it is nearest to
    assert p["match_ptr"][4] == p["match_ptr"][3] + 1 and p["n_far"] == p["n_ambiguous"] == 0 and p["n_not_mutual"] > 0
    assert MC.reference("rules_one_way")["n_not_mutual"] == 0 and MC.reference("rules_any_distance")["n_far"] == 0
    assert MC.reference("rules_any_distance")["n_matches"] >= r["n_matches"]
    r = MC.reference("index_width")
    assert r["nn_best"].tolist() == list(MC.WIDTH_BEST) and r["nn_dist2"].tolist() == [0, 0, 0] and (r["nn_second2"] > 0).all()
    assert r["kp_pairs"].tolist() == [[i, b] for i, b in enumerate(MC.WIDTH_BEST)]
    assert max(MC.CASES, key=lambda n: MC.reference(n)["n_queries"]) == MC.LARGEST[0] and max(MC.CASES, key=lambda n: MC.case(n)[0][-1]) == MC.LARGEST[1]
    assert MC.CHUNK_PAIRS * (MC.WIDTH_N + 3) > MC.CHUNK_ROWS  # the list of test_a_long_pair_list_is_cut_into_chunks does not fit one chunk


def test_premises_of_the_dim_and_flat_limit_cases():
    """Every k-step count the kernel is instantiated for is run by a dim that fills its steps and by one that does not; the flat
    extremes give dim x 255^2 in every instantiation they are stated for."""
    ks = {d: MC.ksteps(d) for d in MC.LIMIT_DIMS}
    assert MC.LIMIT_DIMS == tuple(range(16, 513, 16)) and set(ks.values()) == {1, 2, 4, 8, 16}
    for k in (1, 2, 4, 8, 16):
        assert ks[32 * k] == k and any(v == k and d < 32 * k for d, v in ks.items())  # full, and partial
    assert [ks[d] for d in (64, 80, 144, 240, 256, 272)] == [2, 4, 8, 8, 8, 16]  # upper edges, and just above the one before
    for d in MC.LIMIT_DIMS:
        kp_ptr, desc, pairs, kw = MC.limit_case(f"k{d:03d}")
        assert desc.shape == (115, d) and kp_ptr.tolist() == [0, 70, 115] and pairs.tolist() == [[0, 1], [1, 0]] and kw["ratio"] == 0.95 and kw["mutual"]
    assert {MC.ksteps(d) for d in MC.FLAT_DIMS} == {1, 2, 8, 16} and 496 % MC.KSTEP
    for d in MC.FLAT_DIMS:
        r, top = MC.limit_reference(f"flat{d:03d}"), d * 255 ** 2
        assert (r["nn_dist2"] == top).all() and (r["nn_second2"] == top).all() and (r["nn_best"] == 0).all()
        assert r["kp_pairs"].tolist() == [[0, 0], [0, 0]]
        r = MC.limit_reference(f"flat_one{d:03d}")
        assert (r["nn_best"][:40] == 17).all() and (r["nn_dist2"][:40] == top - 255 ** 2 + 254 ** 2).all() and (r["nn_second2"][:40] == top).all()


def test_premises_of_the_tie_case():
    """On the reference alone: every planted query has exactly the nearest two it was built for, nothing else comes near, every
    pair of TIE_POS occurs in every variant, and among the tied pairs are those the three merges of k_match_nn decide."""
    (kp_ptr, desc, pairs, kw), expect = MC.ties()
    r = MC.limit_reference("ties")
    assert kw["ratio"] is None and not kw["mutual"] and desc.shape[1] == 16 and len(pairs) == 3 * 21 + 2
    assert MC.TIE_NQ > 32 and (MC.TIE_NC + MC.TC - 1) // MC.TC == 3
    by_variant = {}
    for variant, rows, q, best, best2, second2 in expect:
        assert (r["nn_best"][q], r["nn_dist2"][q], r["nn_second2"][q]) == (best, best2, second2), (variant, rows)
        k, l = pairs[q // MC.TIE_NQ]
        D = MR.distance2(desc[kp_ptr[k]:kp_ptr[k + 1]][q % MC.TIE_NQ][None], desc[kp_ptr[l]:kp_ptr[l + 1]])[0]
        assert sorted(np.nonzero(D <= MC.TIE_FAR)[0].tolist()) == sorted(rows)  # the planted rows, and they alone
        by_variant.setdefault(variant, []).append(rows)
    every = sorted((i, j) for a, i in enumerate(MC.TIE_POS) for j in MC.TIE_POS[a + 1:])
    assert len(every) == 231 and all(sorted(by_variant[v]) == every for v in MC.TIE_VARIANTS)
    assert all(sorted(by_variant[v]) == sorted(MC.TIE_TRIPLES) for v in MC.TIE_TRIPLE_VARIANTS)
    assert all(sorted(row // MC.TC for row in t) == [0, 1, 2] for t in MC.TIE_TRIPLES)
    want = {"tie": (9, 9), "near_first": (9, 16), "near_last": (9, 16), "tie3": (9, 9), "mid3": (9, 16)}
    for variant, rows, q, best, best2, second2 in expect:
        assert (best2, second2) == want[variant]
        assert best == {"tie": rows[0], "near_first": rows[0], "near_last": rows[1], "tie3": rows[0], "mid3": rows[1]}[variant]
    waves = {(q % MC.TIE_NQ) // 32 for _, _, q, _, _, _ in expect}
    assert waves == {0, 1}  # planted queries in both waves that take part
    # where the two rows of a tied pair sit (the row-to-(half, register) map), i < j
    same_tile = [(i, j) for i, j in every if i // 32 == j // 32]
    quad = [(i, j) for i, j in same_tile if MC.lane_of_row(i)[0] == MC.lane_of_row(j)[0] and MC.lane_of_row(i)[1] >> 2 == MC.lane_of_row(j)[1] >> 2]
    lane = [(i, j) for i, j in same_tile if MC.lane_of_row(i)[0] == MC.lane_of_row(j)[0] and MC.lane_of_row(i)[1] >> 2 != MC.lane_of_row(j)[1] >> 2]
    upper = [(i, j) for i, j in same_tile if MC.lane_of_row(i)[0] == 1 and MC.lane_of_row(j)[0] == 0]
    upper_far = [(i, j) for i, j in every if i // 32 != j // 32 and MC.lane_of_row(i)[0] == 1 and MC.lane_of_row(j)[0] == 0]
    print(f"tied pairs: {len(quad)} in one register quad, {len(lane)} in one lane across quads, {len(upper)} + {len(upper_far)} with the smaller "
          f"index in the upper half (inside one MFMA tile + across tiles)")
    assert (0, 1) in quad and (4, 7) in quad and (12, 15) in quad and (0, 8) in lane
    assert set(upper) == {(4, 8), (7, 8), (4, 16), (7, 16), (12, 16), (15, 16)} and {(4, 32), (31, 32), (63, 64), (127, 128), (255, 256)} <= set(upper_far)
    assert {(31, 32), (127, 128), (255, 256)} <= set(every)
    assert [MC.lane_of_row(x) for x in (0, 3, 4, 7, 8, 31)] == [(0, 0), (0, 3), (1, 0), (1, 3), (0, 4), (1, 15)]


def test_premises_of_the_wave_and_scan_limit_cases():
    kp_ptr, desc, pairs, kw = MC.limit_case("waves")
    sizes = {(int(kp_ptr[k + 1] - kp_ptr[k]), int(kp_ptr[l + 1] - kp_ptr[l])) for k, l in pairs}
    assert sizes == {(a, b) for a in MC.WAVE_NQ for b in MC.WAVE_NC} and len(pairs) == 27 and desc.shape[1] == 128
    assert MC.WAVE_NQ == tuple(32 * w + e for w in (1, 2, 3) for e in (-1, 0, 1)) and kw["ratio"] == 0.95 and kw["mutual"]
    r = MC.limit_reference("waves")
    assert r["n_matches"] > 0 and r["n_ambiguous"] > 0 and r["n_not_mutual"] > 0
    # more query rows than one trip of the scan's second level: 258 blocks, matches on both sides of block 256
    kp_ptr, desc, pairs, kw = MC.limit_case("scan258")
    r = MC.limit_reference("scan258")
    Q = sum(MC.SCAN_NQ)
    assert Q == r["n_queries"] == MC.SCAN_SUMS * MC.SCAN_BLOCK + MC.SCAN_BLOCK + 1 and (Q + MC.SCAN_BLOCK - 1) // MC.SCAN_BLOCK == 258
    assert np.diff(kp_ptr).tolist() == list(MC.SCAN_NQ) + [MC.SCAN_NC] and desc.shape[1] == 16 and kw["ratio"] == 0.9 and not kw["mutual"]
    kept = np.bincount(np.nonzero(r["code"] == MR.KEPT)[0] // MC.SCAN_BLOCK, minlength=258)
    print(f"scan258: {r['n_matches']} matches, {r['n_ambiguous']} ambiguous; kept in blocks 254 .. 257: {kept[254:].tolist()}")
    assert kept[255] > 0 and kept[256] > 0 and kept[257] == 1 and r["n_ambiguous"] > 0
    assert r["match_ptr"][1] == r["match_ptr"][2] and r["match_ptr"][1] > 0  # the empty image repeats an entry
    assert r["match_ptr"][4] == r["match_ptr"][3] + 1 and r["kp_pairs"][-1].tolist() == [0, 2] and r["dist2"][-1] == 1
    m = MC.limit_reference("scan258_mutual")  # the same rows with the reverse direction: 5 queries against 100 000 and 163 168 candidates
    assert MC.limit_case("scan258_mutual")[3]["mutual"] and m["n_not_mutual"] > 0 and 0 < m["n_matches"] <= 2 * MC.SCAN_NC + 1
    assert m["kp_pairs"][-1].tolist() == [0, 2] and m["nn_best"].tobytes() == r["nn_best"].tobytes()


def _call(lib, n_images, kp_ptr, desc, dim, pairs, n_pairs, ratio=0.8, mutual=1, max_dist2=-1, null=()):
    """mvba_match_descriptors on host arrays, the outputs sized generously; ``null``: the outputs passed as NULL.  Returns
    (rc, message, outputs)."""
    i32, i64, u8 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint8)
    out = {"match_ptr": np.full(16, -7, np.int64), "kp_pairs": np.zeros((16, 2), np.int32), "dist2": np.zeros(16, np.int32),
           "counts": np.full(6, -7, np.int64)}
    ptr = {k: (None if k in null else v.ctypes.data_as(i64 if v.dtype == np.int64 else i32)) for k, v in out.items()}
    rc = lib.mvba_match_descriptors(n_images, None if kp_ptr is None else kp_ptr.ctypes.data_as(i64), None if desc is None else desc.ctypes.data_as(u8),
                                    dim, None if pairs is None else pairs.ctypes.data_as(i32), n_pairs, ratio, mutual, max_dist2, ptr["match_ptr"],
                                    ptr["kp_pairs"], ptr["dist2"], None, None, None, ptr["counts"], None, -1)
    return rc, lib.mvba_last_error().decode(), out


def test_library_exports_match_descriptors_and_checks_its_arguments():
    """The symbol of include/mvba.h exists in libmvba.so with its prototype bound, and every argument error comes back before any
    device work, with the number in its message: no GPU is needed.  So do the complete answers of the calls that ask nothing."""
    assert "mvba_match_descriptors" in _mvba.SIGNATURES and len(_mvba.SIGNATURES["mvba_match_descriptors"][1]) == 18
    if not os.path.exists(_mvba.LIB_PATH):
        pytest.skip("libmvba.so is not built")
    assert hasattr(ctypes.CDLL(_mvba.LIB_PATH), "mvba_match_descriptors")
    lib = _mvba.load_library()
    kp = np.array([0, 2, 2, 5], np.int64)
    desc = np.zeros((5, 32), np.uint8)
    pr = np.array([[0, 2], [2, 0]], np.int32)
    bad = _mvba.MVBA_ERR_BADARG

    def msg(*a, **k):
        return _call(lib, *a, **k)[:2]
    for name, pos in (("match_ptr", 10), ("kp_pairs", 11), ("dist2", 12), ("counts", 16)):
        assert msg(3, kp, desc, 32, pr, 2, null=(name,)) == (bad, f"null argument: {name} (argument {pos})")
    assert msg(3, None, desc, 32, pr, 2) == (bad, "null argument: kp_ptr (argument 2)")
    assert msg(3, kp, None, 32, pr, 2) == (bad, "null argument: desc (argument 3) with 5 keypoints")
    assert msg(3, kp, desc, 32, None, 2) == (bad, "null argument: pairs (argument 5) with n_pairs = 2")
    assert msg(3, kp, desc, 32, pr, -1) == (bad, "n_pairs = -1: negative size")
    assert msg(0, kp, desc, 32, pr, 2) == (bad, "n_images = 0 must be at least 1")
    assert msg(2, np.array([1, 2, 3], np.int64), desc, 32, pr, 0) == (bad, "kp_ptr[0] = 1 must be 0")
    assert msg(3, np.array([0, 3, 2, 5], np.int64), desc, 32, pr, 2) == (bad, "kp_ptr is not ascending: kp_ptr[2] = 2 after 3")
    assert msg(1, np.array([0, 2 ** 31], np.int64), desc, 32, pr, 0) == (bad, "n_nodes = kp_ptr[n_images] = 2147483648 must be < 2^31")
    for dim in (0, 8, 24, 520, 528, -16):
        assert msg(3, kp, desc, dim, pr, 2) == (bad, f"dim = {dim} must be a multiple of 16 in 16 .. 512")
    for ratio, text in ((-0.1, "-0.100000"), (1.5, "1.500000"), (float("nan"), "nan")):
        rc, m = msg(3, kp, desc, 32, pr, 2, ratio=ratio)
        assert rc == bad and m.replace("-nan", "nan") == f"ratio = {text} must be in (0, 1], or 0 for no ratio test"
    assert msg(3, kp, desc, 32, np.array([[0, 2], [3, 0]], np.int32), 2) == (bad, "pairs[1][0] = 3: image index out of range, n_images = 3")
    assert msg(3, kp, desc, 32, np.array([[0, -1]], np.int32), 1) == (bad, "pairs[0][1] = -1: image index out of range, n_images = 3")
    assert msg(3, kp, desc, 32, np.array([[0, 2], [2, 2]], np.int32), 2) == (bad, "pairs[1] = (2, 2): an image is not matched with itself")
    huge = np.array([0, 2 ** 30, 2 ** 30 + 1], np.int64)  # two pairs of 2^30 queries each
    assert msg(2, huge, desc, 32, np.array([[0, 1], [0, 1]], np.int32), 2) == (bad, "Q = 2147483648 queries up to pair 1: the sum over the pairs must be < 2^31")
    # nothing asked: complete answers, no device work
    rc, _, out = _call(lib, 3, kp, desc, 32, None, 0)
    assert rc == _mvba.MVBA_OK and out["match_ptr"][0] == 0 and out["counts"].tolist() == [0] * 6
    rc, _, out = _call(lib, 3, kp, desc, 32, np.array([[1, 0], [1, 2]], np.int32), 2)  # every query image is empty
    assert rc == _mvba.MVBA_OK and out["match_ptr"][:3].tolist() == [0, 0, 0] and out["counts"].tolist() == [0] * 6
    rc, _, out = _call(lib, 1, np.zeros(2, np.int64), None, 128, None, 0)  # no keypoints at all: desc is not looked at
    assert rc == _mvba.MVBA_OK


def test_match_descriptors_fails_loudly_without_gpu():
    if os.path.exists(_mvba.LIB_PATH) and _mvba.device_count() > 0:
        pytest.skip("a device is visible")
    kp_ptr, desc, pairs, _ = MC.case("rules")
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        match_descriptors((kp_ptr, desc), pairs)
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        _mvba.match_descriptors(kp_ptr, desc, pairs)


def test_input_forms_and_their_errors():
    sd = MC.scene_descriptors()
    kp_ptr, desc = descriptor_arrays(sd.descriptors)
    assert kp_ptr.dtype == np.int64 and desc.dtype == np.uint8 and desc.flags.c_contiguous and kp_ptr[0] == 0 and kp_ptr[-1] == len(desc)
    for i in (0, 3, 7):
        np.testing.assert_array_equal(desc[kp_ptr[i]:kp_ptr[i + 1]], sd.descriptors[i])
    again = descriptor_arrays((kp_ptr, desc))
    np.testing.assert_array_equal(again[0], kp_ptr)
    np.testing.assert_array_equal(again[1], desc)
    with pytest.raises(ValueError, match=r"descriptors\[1\] has dtype float32; descriptors must be uint8.  Quantise"):
        match_descriptors([sd.descriptors[0], sd.descriptors[1].astype(np.float32)])
    with pytest.raises(ValueError, match="desc has dtype int64"):
        match_descriptors((kp_ptr, desc.astype(np.int64)))
    with pytest.raises(ValueError, match=r"different dim: \[64, 128\]"):
        match_descriptors([sd.descriptors[0], sd.descriptors[1][:, :64]])
    with pytest.raises(ValueError, match="kp_ptr must ascend"):
        match_descriptors((np.array([0, 3, 2]), desc[:2]))
    with pytest.raises(ValueError, match=r"pair \(0, 1\) is listed twice"):
        match_descriptors(sd.descriptors, pairs=[(0, 1), (1, 0), (0, 1)])
    for ratio in (0.0, 1.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match="ratio = .* must be in"):
            match_descriptors(sd.descriptors, ratio=ratio)
    with pytest.raises(ValueError, match="max_distance = -1.0 must be >= 0"):
        match_descriptors(sd.descriptors, max_distance=-1.0)
    if os.path.exists(_mvba.LIB_PATH) and _mvba.device_count() > 0:  # what the ABI refuses comes back as a ValueError too
        with pytest.raises(ValueError, match="image index out of range"):
            match_descriptors(sd.descriptors, pairs=[(0, 8)])


def test_premise_of_the_end_to_end_case():
    """Whatever the seed: the reference finds most of the true matches, lets wrong ones through, and its ratio test removes most
    of those.  (Seed 25: the figures are printed.)"""
    sd = MC.scene_descriptors()
    assert len(MC.scene_pairs()) == 28 and all(d.shape == (len(k), 128) for d, k in zip(sd.descriptors, sd.mo.keypoints))
    assert (sd.twin != np.arange(len(sd.twin))).sum() == MC.E2E_TWINS
    for (k, l), idx in sd.mo.matches.items():  # the true matches join keypoints of one point
        assert (sd.point_of_kp[k][idx[:, 0]] == sd.point_of_kp[l][idx[:, 1]]).all() and (sd.point_of_kp[k][idx[:, 0]] >= 0).all()
    with_ratio, without = MC.scene_reference(MC.E2E_RATIO), MC.scene_reference(None)
    t1, s1, o1, n_true = MC.scene_score(with_ratio)
    t0, s0, o0, _ = MC.scene_score(without)
    print(f"ratio {MC.E2E_RATIO}: {t1 + s1 + o1} matches, {t1} true of {n_true}, {s1} between twins, {o1} other wrong; "
          f"no ratio: {t0 + s0 + o0} matches, {t0} true, {s0} between twins, {o0} other wrong")
    assert t1 >= 0.85 * n_true
    assert s1 + o1 >= 1
    assert s1 + o1 < 0.5 * (s0 + o0)
