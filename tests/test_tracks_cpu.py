"""Feature tracks from pairwise matches, the parts that need no GPU: the NumPy reference against scipy's connected
components on every case, the premises of the GPU cases, the exported symbol with its argument errors, the input forms of
build_tracks, the lists verify_matches builds, and the premise of the end-to-end GPU test."""
import ctypes
import os

import numpy as np
import pytest

from lib import _mvba
from lib.initialization import build_tracks, match_graph, match_pair_lists, verify_matches

import _ransac_ref as RR
import _tracks_cases as TC
import _tracks_ref as TR


@pytest.mark.parametrize("name", sorted(TC.GRAPHS) + ["scene"])
def test_reference_labels_against_scipy(name):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import coo_matrix

    if name == "scene":
        mo = TC.scene_matches(TC.INVARIANCE_WRONG)
        kp_ptr, _, edges, _, _ = match_graph(mo.keypoints, mo.matches)
        ok = None
    else:
        kp_ptr, _, edges, ok, _ = TC.graph(name)
    _labels_against_scipy(csgraph, coo_matrix, kp_ptr, edges, ok)


@pytest.mark.parametrize("name", sorted(TC.LIMIT_GRAPHS))
def test_limit_reference_labels_against_scipy(name):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import coo_matrix

    kp_ptr, _, edges, ok, _ = TC.limit_graph(name)
    _labels_against_scipy(csgraph, coo_matrix, kp_ptr, edges, ok)


def _labels_against_scipy(csgraph, coo_matrix, kp_ptr, edges, ok):
    n = int(kp_ptr[-1])
    used = edges if ok is None else edges[ok != 0]
    label = TR.labels(n, used)
    _, comp = csgraph.connected_components(coo_matrix((np.ones(len(used)), (used[:, 0], used[:, 1])), shape=(n, n)), directed=False)
    first = np.full(comp.max() + 1 if n else 0, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))  # scipy numbers the components as it likes: the smallest node of each
    np.testing.assert_array_equal(label, first[comp])


def test_premises_of_the_hand_made_cases():
    for name, want in TC.NODE_TRACK.items():
        assert TC.reference(name)["node_track"].tolist() == want, name
    r = TC.reference("tiny")
    assert (r["n_conflicting"], r["n_conflicting_nodes"], r["n_tracks"]) == (1, 3, 1) and r["cam_idx"].tolist() == [0, 1, 2]
    r = TC.reference("blocks")
    assert r["n_tracks"] == TC.BLOCK + 1 and (np.diff(r["pt_ptr"]) == 3).all() and len(TC.graph("blocks")[2]) > 2 * TC.BLOCK
    r, m = TC.reference("path130"), len(TC.graph("path130")[0]) - 1
    assert m == 130 and sorted(np.diff(r["pt_ptr"]).tolist()) == [3, 130] and r["n_oversize"] == 0  # exactly n_images: kept
    r, m = TC.reference("path131"), len(TC.graph("path131")[0]) - 1
    assert m == 130 and (r["n_oversize"], r["n_oversize_nodes"], r["n_tracks"]) == (1, 131, 1)  # one more: dropped, the side track stays
    assert (r["node_track"] == -3).sum() == 131 and (r["node_track"] == 0).sum() == 3
    r = TC.reference("sort32")
    assert sorted(np.diff(r["pt_ptr"]).tolist()) == [31, 32, 33, 64, 65]
    for a in range(5):  # ascending in camera, one keypoint per image
        assert (np.diff(r["cam_idx"][r["pt_ptr"][a]:r["pt_ptr"][a + 1]]) > 0).all()
    r = TC.reference("hub")
    assert (r["n_oversize"], r["n_oversize_nodes"], r["n_tracks"], r["n_obs"]) == (1, 5001, 1, 2)
    r = TC.reference("messy")
    assert set(r["node_track"].tolist()) == {0, -1, -2, -3} and (r["n_short"], r["n_conflicting"], r["n_singletons"]) == (1, 1, 3)
    kp_ptr, kp_xy, edges, ok, ml = TC.graph("messy")
    assert kp_ptr[2] == kp_ptr[3] and ml == 3 and (ok == 0).sum() == 1
    assert TR.build_tracks(kp_ptr, kp_xy, edges, None, ml)["n_conflicting"] == 2  # the masked edge WOULD cause a conflict
    r = TC.reference("empty")
    assert r["pt_ptr"].tolist() == [0] and r["n_tracks"] == 0 and len(r["node_track"]) == 0
    r = TC.reference("path4096")
    assert r["pt_ptr"].tolist() == [0, 4096] and r["cam_idx"].tolist() == list(range(4096))


def test_premises_of_the_big_limit_graphs():
    """More than 256 scan blocks of nodes with roots of every class on both sides of node 262 144 (in both scans: candidates, and
    survivors), and in the long form more edges than one sweep of the hook kernel's grid -- the same edge SET, the same answer."""
    kp_ptr, _, edges, ok, min_length = TC.limit_graph("big")
    _, _, long_edges, _, _ = TC.limit_graph("big_long")
    n, second_trip = int(kp_ptr[-1]), TC.SCAN_SUMS * TC.SCAN_BLOCK
    assert n > second_trip + TC.SCAN_BLOCK and len(kp_ptr) - 1 == 6 and min_length == 3 and ok is None
    assert 0 < len(edges) < TC.HOOK_EDGES < len(long_edges) == (TC.BIG_COPIES + 1) * len(edges)
    as_set = lambda e: np.unique(e.min(axis=1).astype(np.int64) * n + e.max(axis=1))
    np.testing.assert_array_equal(as_set(edges), as_set(long_edges))
    assert (long_edges[:, 0] < long_edges[:, 1]).any() and (long_edges[:, 0] > long_edges[:, 1]).any()
    r, rl = TC.limit_reference("big"), TC.limit_reference("big_long")
    for key in ("pt_ptr", "cam_idx", "obs_node", "xy", "node_track"):
        assert r[key].tobytes() == rl[key].tobytes(), key
    assert all(r[k] == rl[k] for k in TR.COUNTS) and all(r[k] > 0 for k in TR.COUNTS)
    label, size = r["label"], np.bincount(r["label"], minlength=n)
    roots = np.nonzero(label == np.arange(n))[0]
    code = r["node_track"][roots]
    classes = {"survivor": code >= 0, "conflict": (code == -3) & (size[roots] <= 6), "oversize": (code == -3) & (size[roots] > 6),
               "short": code == -2, "singleton": code == -1}
    block = roots // TC.SCAN_BLOCK
    for name, of in classes.items():
        counts = [int((of & (block < TC.SCAN_SUMS)).sum()), int((of & (block >= TC.SCAN_SUMS)).sum())]
        print(f"big: {name} roots below node {second_trip}, from it on: {counts}")
        assert min(counts) > 0, name


def test_premises_of_the_small_limit_graphs():
    # long tracks in every wave of the sort, at lanes 0 and 63, three of them in one wave among short ones
    r = TC.limit_reference("sort_waves")
    lengths = np.diff(r["pt_ptr"])
    assert r["n_tracks"] == TC.SORT_N == len(lengths) and r["obs_node"][r["pt_ptr"][:-1]].tolist() == list(range(TC.SORT_N))  # candidate c is track c
    assert all(lengths[c] == L for c, L in TC.SORT_LONG.items()) and set(TC.SORT_LONG.values()) == {33, 40, 64, 65, 70}
    short = np.delete(lengths, list(TC.SORT_LONG))
    assert set(short.tolist()) == {2, 3} and min(TC.SORT_LONG.values()) > TC.LANE_MAX
    place = [(c // TC.BLOCK, c % TC.BLOCK // 64, c % 64) for c in TC.SORT_LONG]  # (workgroup, wave, lane)
    assert {p[:2] for p in place} == {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0)} and {0, 1, 62, 63} <= {p[2] for p in place}
    assert sum(p[:2] == (0, 0) for p in place) == 3 and sum(p[:2] == (0, 1) for p in place) == 3
    assert TC.SORT_LONG[max(TC.SORT_LONG)] == max(TC.SORT_LONG.values()) == TC.SORT_M
    for a in range(r["n_tracks"]):
        assert (np.diff(r["cam_idx"][r["pt_ptr"][a]:r["pt_ptr"][a + 1]]) > 0).all()
    # empty images first, last, and two in a row
    kp_ptr = TC.limit_graph("ends")[0]
    r = TC.limit_reference("ends")
    assert kp_ptr[0] == kp_ptr[1] and kp_ptr[3] == kp_ptr[4] == kp_ptr[5] and kp_ptr[-2] == kp_ptr[-1] and len(kp_ptr) - 1 == 8
    assert r["node_track"].tolist() == TC.LIMIT_NODE_TRACK["ends"] and r["cam_idx"].tolist() == TC.LIMIT_CAM_IDX["ends"]
    # neighbouring segments that meet in one image: the sorted buffer of the candidates, restated
    kp_ptr, _, edges, _, _ = TC.limit_graph("stairs")
    r = TC.limit_reference("stairs")
    n = int(kp_ptr[-1])
    label = r["label"]
    buf = np.lexsort((np.arange(n), label))  # every component is a candidate here
    image = np.searchsorted(kp_ptr, buf, side="right") - 1
    meet = np.nonzero((image[1:] == image[:-1]) & (label[buf][1:] != label[buf][:-1]))[0] + 1  # p: entries p - 1 | p
    assert meet.tolist() == list(range(2, 2 * TC.STAIR_K + 1, 2)) and TC.BLOCK in meet  # every boundary, entry 255 | 256 among them
    assert (buf[meet] > buf[meet - 1]).any() and (buf[meet] < buf[meet - 1]).any()  # either order of the two inside their image
    assert (r["n_tracks"], r["n_conflicting"], r["n_conflicting_nodes"], r["n_singletons"]) == (TC.STAIR_K, 1, 3, 0)
    assert (r["node_track"][buf[-3:]] == -3).all() and (np.diff(r["pt_ptr"]) == 2).all()


def _call(lib, n_images, kp_ptr, kp_xy, edges, n_edges, ok, min_length, null=()):
    """mvba_build_tracks on host arrays, the outputs sized as the header says; ``null``: the outputs passed as NULL."""
    i32, i64, u8 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint8)
    n = 16
    out = {"pt_ptr": np.zeros(n, np.int64), "cam_idx": np.zeros(n, np.int32), "obs_node": np.zeros(n, np.int32), "xy": np.zeros((n, 2)),
           "node_track": np.zeros(n, np.int32), "counts": np.zeros(10, np.int64)}
    ptr = {k: (None if k in null else v.ctypes.data_as({np.dtype(np.int64): i64, np.dtype(np.int32): i32}.get(v.dtype, _mvba._dp)))
           for k, v in out.items()}
    rc = lib.mvba_build_tracks(n_images, None if kp_ptr is None else kp_ptr.ctypes.data_as(i64), None if kp_xy is None else _mvba._ptr(kp_xy),
                               None if edges is None else edges.ctypes.data_as(i32), n_edges, None if ok is None else ok.ctypes.data_as(u8),
                               min_length, ptr["pt_ptr"], ptr["cam_idx"], ptr["obs_node"], ptr["xy"], ptr["node_track"], ptr["counts"], None, -1)
    return rc, lib.mvba_last_error().decode()


def test_library_exports_build_tracks_and_checks_its_arguments():
    """The symbol of include/mvba.h exists in libmvba.so with its prototype bound, and every argument error comes back before
    any device work, with the number in its message: no GPU is needed."""
    assert "mvba_build_tracks" in _mvba.SIGNATURES and len(_mvba.SIGNATURES["mvba_build_tracks"][1]) == 15
    if not os.path.exists(_mvba.LIB_PATH):
        pytest.skip("libmvba.so is not built")
    assert hasattr(ctypes.CDLL(_mvba.LIB_PATH), "mvba_build_tracks")
    lib = _mvba.load_library()
    kp = np.array([0, 2, 2, 5], np.int64)
    kxy = np.zeros((5, 2))
    e = np.array([[0, 4], [3, 3], [4, 1]], np.int32)
    bad = _mvba.MVBA_ERR_BADARG
    for name, pos in (("pt_ptr", 8), ("cam_idx", 9), ("obs_node", 10), ("node_track", 12), ("counts", 13)):
        assert _call(lib, 3, kp, kxy, e, 3, None, 2, null=(name,)) == (bad, f"null argument: {name} (argument {pos})")
    assert _call(lib, 3, None, kxy, e, 3, None, 2) == (bad, "null argument: kp_ptr (argument 2)")
    assert _call(lib, 3, kp, None, e, 3, None, 2) == (bad, "null argument: kp_xy (argument 3) with an xy to fill")
    assert _call(lib, 3, kp, kxy, None, 3, None, 2) == (bad, "null argument: edges (argument 4) with n_edges = 3")
    assert _call(lib, 0, kp, kxy, e, 3, None, 2) == (bad, "n_images = 0 must be at least 1")
    assert _call(lib, 2, np.array([1, 2, 3], np.int64), kxy, e, 3, None, 2) == (bad, "kp_ptr[0] = 1 must be 0")
    assert _call(lib, 3, np.array([0, 3, 2, 5], np.int64), kxy, e, 3, None, 2) == (bad, "kp_ptr is not ascending: kp_ptr[2] = 2 after 3")
    assert _call(lib, 1, np.array([0, 2 ** 31], np.int64), kxy, e, 0, None, 2) == (bad, "n_nodes = kp_ptr[n_images] = 2147483648 must be < 2^31")
    assert _call(lib, 3, kp, kxy, e, -1, None, 2) == (bad, "n_edges = -1: negative size")
    assert _call(lib, 3, kp, kxy, e, 3, None, 1) == (bad, "min_length = 1 must be at least 2")
    assert _call(lib, 3, kp, kxy, np.array([[0, 4], [5, 1]], np.int32), 2, None, 2) == (bad, "edges[1][0] = 5: node id out of range, n_nodes = 5")
    assert _call(lib, 3, kp, kxy, np.array([[0, 4], [2, -1]], np.int32), 2, None, 2) == (bad, "edges[1][1] = -1: node id out of range, n_nodes = 5")
    # no keypoints at all: nothing for the device to do, and the answer is complete
    rc, _ = _call(lib, 2, np.zeros(3, np.int64), kxy, None, 0, None, 2)
    assert rc == _mvba.MVBA_OK


def test_build_tracks_fails_loudly_without_gpu():
    if os.path.exists(_mvba.LIB_PATH) and _mvba.device_count() > 0:
        pytest.skip("a device is visible")
    mo = TC.scene_matches(0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        build_tracks(mo.keypoints, mo.matches)
    with pytest.raises(RuntimeError, match="no CPU fallback|not found"):
        verify_matches(mo.keypoints, mo.matches, TC.E2E_THRESHOLD)


def test_input_forms_give_the_same_nodes_and_edges():
    mo = TC.scene_matches(TC.INVARIANCE_WRONG)
    kp_ptr, kp_xy, edges, ip, kp = match_graph(mo.keypoints, mo.matches)  # a list of keypoint arrays, a dict of matches
    assert kp_ptr.dtype == np.int64 and edges.dtype == np.int32 and kp_ptr[0] == 0 and kp_ptr[-1] == len(kp_xy) == sum(len(a) for a in mo.keypoints)
    for i in (0, 3, 7):
        np.testing.assert_array_equal(kp_xy[kp_ptr[i]:kp_ptr[i + 1]], mo.keypoints[i])
    assert len(edges) == mo.n_true + mo.n_wrong
    at = 0
    for (k, l), idx in mo.matches.items():  # numbered in the dict's order
        np.testing.assert_array_equal(ip[at:at + len(idx)], np.tile([k, l], (len(idx), 1)))
        np.testing.assert_array_equal(edges[at:at + len(idx)], np.stack([kp_ptr[k] + idx[:, 0], kp_ptr[l] + idx[:, 1]], axis=1))
        at += len(idx)
    for form in ((mo.keypoints, (ip, kp)), ((kp_ptr, kp_xy), mo.matches), ((kp_ptr, kp_xy), (ip.tolist(), kp.tolist()))):
        got = match_graph(*form)
        for a, b in zip(got, (kp_ptr, kp_xy, edges, ip, kp)):
            np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match=r"match 1 is between images \(0, 8\)"):
        match_graph(mo.keypoints, (np.array([[0, 1], [0, 8]]), np.array([[0, 0], [0, 0]])))
    with pytest.raises(ValueError, match=r"match 0 joins keypoints \(0, \d+\) of images \(0, 1\)"):
        match_graph(mo.keypoints, {(0, 1): np.array([[0, len(mo.keypoints[1])]])})
    with pytest.raises(ValueError, match="kp_ptr must ascend"):
        match_graph((np.array([0, 3, 2]), np.zeros((2, 2))), {})


def test_verify_matches_builds_one_two_camera_list_per_pair():
    kps = [np.arange(8.0).reshape(4, 2), np.zeros((0, 2)), 100 + np.arange(6.0).reshape(3, 2), 200 + np.arange(4.0).reshape(2, 2)]
    matches = {(0, 2): np.array([[0, 1], [3, 2]]), (3, 2): np.array([[1, 0]]), (2, 0): np.array([[2, 1]]), (2, 2): np.array([[0, 1]])}
    pairs, lists, n = match_pair_lists(kps, matches)
    assert n == 5 and pairs.tolist() == [[0, 2], [2, 3]]  # (2, 0) is (0, 2) turned round; (2, 2) belongs to no pair
    ids, ptr, cam, xy = lists[0]
    assert ids.tolist() == [0, 1, 3] and ptr.tolist() == [0, 2, 4, 6] and cam.tolist() == [0, 2] * 3 and cam.dtype == np.int32
    np.testing.assert_array_equal(xy, [kps[0][0], kps[2][1], kps[0][3], kps[2][2], kps[0][1], kps[2][2]])
    ids, ptr, cam, xy = lists[1]
    assert ids.tolist() == [2] and ptr.tolist() == [0, 2] and cam.tolist() == [2, 3]
    np.testing.assert_array_equal(xy, [kps[2][0], kps[3][1]])  # camera k < l first: the match was given as (3, 2)
    with pytest.raises(ValueError, match="model must be"):
        verify_matches(kps, matches, 0.01, model="affine")


@pytest.fixture(scope="module")
def verified_on_the_host():
    """verify_matches of the end-to-end case with the CPU RANSAC reference in the place of the device call."""
    mo = TC.scene_matches(TC.E2E_WRONG)
    pairs, lists, n = match_pair_lists(mo.keypoints, mo.matches)
    ok = np.zeros(n, bool)
    for p, (ids, ptr, cam, xy) in enumerate(lists):
        out = RR.two_view_robust(ptr, cam, xy, 8, pairs[p:p + 1], TC.E2E_THRESHOLD, TC.E2E_HYP, TC.E2E_SEED, 2)
        if out["status"][0] == 0:
            ok[ids] = out["inlier"][0]
    return mo, ok


def test_premise_of_the_end_to_end_case(verified_on_the_host):
    mo, ok = verified_on_the_host
    wrong = np.concatenate([mo.wrong[kl] for kl in mo.matches])
    assert len(mo.matches) == 28 and mo.n_wrong == round(TC.E2E_WRONG * mo.n_true) == wrong.sum()
    kp_ptr, kp_xy, edges, _, _ = match_graph(mo.keypoints, mo.matches)
    r = TR.build_tracks(kp_ptr, kp_xy, edges, ok)
    share = TC.foreign_share(mo, r["cam_idx"], r["obs_node"] - kp_ptr[r["cam_idx"]], r["pt_ptr"])
    plain = TR.build_tracks(kp_ptr, kp_xy, edges)
    print(f"wrong matches kept {int((ok & wrong).sum())} of {int(wrong.sum())}, true ones kept {int((ok & ~wrong).sum())} of {int((~wrong).sum())}; "
          f"tracks {r['n_tracks']} ({plain['n_tracks']} unverified), foreign share {share:.4f}")
    assert (ok & ~wrong).sum() >= 0.99 * (~wrong).sum()
    assert r["n_tracks"] >= TC.E2E_MIN_TRACKS and share <= TC.E2E_MAX_FOREIGN
    assert plain["n_tracks"] < TC.E2E_MIN_TRACKS  # without the verification the wrong matches chain the tracks together
