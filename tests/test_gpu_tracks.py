"""Feature tracks from pairwise matches on the device: mvba_build_tracks against the NumPy reference
(tests/_tracks_ref.py) on the hand-made graphs of tests/_tracks_cases.py and the limit graphs beside them -- every comparison exact: integers, and xy bit for bit --,
its invariance under a restatement of the edge set, the recovery of a scene's observation list, and matches with wrong ones among
them through verify_matches, build_tracks, bootstrap and Huber bundle adjustment."""
import numpy as np
import pytest

from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster
from lib.initialization import bootstrap, build_tracks, covisibility, verify_matches

import _tracks_cases as TC
import _tracks_ref as TR

pytestmark = pytest.mark.gpu

ARRAYS = ("pt_ptr", "cam_idx", "obs_node", "xy", "node_track")


def _same(got, want, what):
    for key in ARRAYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        assert got[key].tobytes() == want[key].tobytes(), (what, key)
    for key in TR.COUNTS:
        assert got[key] == want[key], (what, key, got[key], want[key])


@pytest.mark.parametrize("name", sorted(TC.GRAPHS))
def test_hand_made_graph_matches_the_reference(name):
    kp_ptr, kp_xy, edges, ok, min_length = TC.graph(name)
    got = _mvba.build_tracks(kp_ptr, kp_xy, edges, edge_ok=ok, min_length=min_length)
    _same(got, TC.reference(name), name)
    print(f"{name}: {got['n_rounds']} rounds, timings {got['timings_ms']}")
    assert got["n_rounds"] >= (1 if len(edges) else 0)
    if name in TC.NODE_TRACK:
        assert got["node_track"].tolist() == TC.NODE_TRACK[name]
    if name == "empty":
        assert got["pt_ptr"].tolist() == [0] and got["n_tracks"] == 0
    if name == "sort32":
        for a in range(got["n_tracks"]):
            assert (np.diff(got["cam_idx"][got["pt_ptr"][a]:got["pt_ptr"][a + 1]]) > 0).all()
    np.testing.assert_array_equal(got["xy"], kp_xy[got["obs_node"]])
    # without coordinates: the same integers, and no xy
    bare = _mvba.build_tracks(kp_ptr, None, edges, edge_ok=ok, min_length=min_length)
    assert bare["xy"] is None and all(bare[k].tobytes() == got[k].tobytes() for k in ARRAYS if k != "xy")


@pytest.mark.parametrize("name", sorted(TC.LIMIT_GRAPHS))
def test_limit_graph_matches_the_reference(name):
    """The limits pass of DESIGN.md §24: more nodes than the scan's second level takes in one trip and more edges than one sweep
    of the hook kernel's grid, long tracks in every wave of the sort, empty images at both ends, and neighbouring segments that
    meet in one image.  What each graph is for is asserted on the reference alone in tests/test_tracks_cpu.py."""
    kp_ptr, kp_xy, edges, ok, min_length = TC.limit_graph(name)
    got = _mvba.build_tracks(kp_ptr, kp_xy, edges, edge_ok=ok, min_length=min_length)
    print(f"{name}: {len(edges)} edges, {got['n_rounds']} rounds, timings {got['timings_ms']}")
    _same(got, TC.limit_reference(name), name)
    np.testing.assert_array_equal(got["xy"], kp_xy[got["obs_node"]])
    if name in TC.LIMIT_NODE_TRACK:
        assert got["node_track"].tolist() == TC.LIMIT_NODE_TRACK[name] and got["cam_idx"].tolist() == TC.LIMIT_CAM_IDX[name]
    if name == "big_long":  # the edge set of "big", restated: byte for byte the same answer
        plain = TC.limit_reference("big")
        assert all(got[k].tobytes() == plain[k].tobytes() for k in ARRAYS)
    if name == "sort_waves":
        assert got["n_tracks"] == TC.SORT_N
        for a in range(got["n_tracks"]):
            assert (np.diff(got["cam_idx"][got["pt_ptr"][a]:got["pt_ptr"][a + 1]]) > 0).all()
    if name == "stairs":
        assert (got["n_tracks"], got["n_conflicting"], got["n_conflicting_nodes"]) == (TC.STAIR_K, 1, 3)


def test_no_edges_leaves_every_keypoint_unmatched():
    kp_ptr, kp_xy, _, _, _ = TC.graph("blocks")
    got = _mvba.build_tracks(kp_ptr, kp_xy, np.zeros((0, 2), np.int32))
    assert got["n_tracks"] == 0 and got["n_rounds"] == 0 and got["n_singletons"] == kp_ptr[-1] and (got["node_track"] == -1).all()
    assert got["pt_ptr"].tolist() == [0] and len(got["cam_idx"]) == 0


def test_outputs_depend_on_the_edge_set_alone():
    """The scene's matches with 3 % wrong ones, as they come, permuted and turned round, and partly duplicated: every output array is
    bitwise the same, and the same again in a second call."""
    keypoints, forms = TC.invariance_inputs()
    runs = [build_tracks(keypoints, f) for f in forms] + [build_tracks(keypoints, forms[0])]
    first = runs[0]
    from lib.initialization import match_graph

    kp_ptr, kp_xy, edges, _, _ = match_graph(keypoints, forms[0])
    want = TR.build_tracks(kp_ptr, kp_xy, edges)
    assert first[3]["n_conflicting"] + first[3]["n_oversize"] > 0  # (the wrong matches do something)
    for i, (pt_ptr, cam_idx, xy, info) in enumerate(runs):
        _same({"pt_ptr": pt_ptr, "cam_idx": cam_idx, "xy": xy, **info}, want, f"input {i}")
        np.testing.assert_array_equal(info["kp_idx"], first[3]["kp_idx"])


def test_clean_matches_return_the_scene():
    """Without wrong matches the tracks ARE the scene's observation list, in the order of each point's first keypoint: xy bit for
    bit, and kp_idx undoes the shuffle of the keypoints."""
    sc, mo = TC.scene(), TC.scene_matches(0.0)
    pt_ptr, cam_idx, xy, info = build_tracks(mo.keypoints, mo.matches)
    assert info["n_tracks"] == sc.n_points and info["n_obs"] == sc.n_obs and info["n_conflicting"] == info["n_oversize"] == info["n_short"] == 0
    assert info["n_singletons"] == 8 * 5  # the extra keypoints
    # the scene's points in the order the contract fixes: by the node of their first observation
    first_node = info["kp_ptr"][sc.cam_idx[sc.pt_ptr[:-1]]] + mo.kp_of_obs[sc.pt_ptr[:-1]]
    order = np.argsort(first_node)
    obs = np.concatenate([np.arange(sc.pt_ptr[a], sc.pt_ptr[a + 1]) for a in order])
    np.testing.assert_array_equal(np.diff(pt_ptr), np.diff(sc.pt_ptr)[order])
    np.testing.assert_array_equal(cam_idx, sc.cam_idx[obs])
    assert xy.tobytes() == np.ascontiguousarray(sc.xy[obs]).tobytes()
    np.testing.assert_array_equal(info["kp_idx"], mo.kp_of_obs[obs])
    count = covisibility(pt_ptr, cam_idx, 8)  # the list goes to the other entry points as it is
    np.testing.assert_array_equal(np.diag(count), np.bincount(sc.cam_idx, minlength=8))


def _huber_cost(n, pt_ptr, cam, xy, X, K, R, t, delta):
    eng = _mvba.HipEngine(n, 8, pt_ptr, cam, xy, 1.0, "x-up_z-forward", loss="huber", loss_scale=delta)
    eng.set_params(X, K[:, 0, 0], K[:, :2, 2], t, R)
    E = eng.cost()
    eng.close()
    return E


def test_matches_to_bundle_adjustment():
    """The scene's matches with a tenth as many wrong ones added: verified pair by pair, built into tracks, bootstrapped with the
    three robust thresholds and bundle-adjusted under the Huber loss.  All 8 cameras are registered and the final cost is below
    that of the ground truth on the same list (the premise is tests/test_tracks_cpu.py::test_premise_of_the_end_to_end_case)."""
    sc, mo = TC.scene(), TC.scene_matches(TC.E2E_WRONG)
    ok, vi = verify_matches(mo.keypoints, mo.matches, TC.E2E_THRESHOLD, n_hypotheses=TC.E2E_HYP, seed=TC.E2E_SEED)
    assert set(ok) == set(mo.matches) and (vi["status"] == 0).all() and len(vi["pairs"]) == 28
    wrong = np.concatenate([mo.wrong[kl] for kl in mo.matches])
    kept = np.concatenate([ok[kl] for kl in mo.matches])
    pt_ptr, cam_idx, xy, info = build_tracks(mo.keypoints, mo.matches, match_ok=ok)
    share = TC.foreign_share(mo, cam_idx, info["kp_idx"], pt_ptr)
    print(f"wrong matches kept {int((kept & wrong).sum())} of {int(wrong.sum())}; tracks {info['n_tracks']}, foreign share {share:.4f}")
    assert info["n_tracks"] >= TC.E2E_MIN_TRACKS and share <= TC.E2E_MAX_FOREIGN
    thr = TC.E2E_THRESHOLD
    K, R, t, X, bi = bootstrap(pt_ptr, cam_idx, xy, sc.init_K, ransac_threshold=thr, pose_threshold=thr, triangulate_threshold=thr,
                               n_hypotheses=TC.E2E_HYP, seed=TC.E2E_SEED)
    assert bi["camera_ok"].all() and len(bi["order"]) == 8
    # the list the points were triangulated from, points renumbered; the ground truth of a track: the scene point most of it belongs to
    truth = TC.track_points(mo, cam_idx, info["kp_idx"], pt_ptr)[0]
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    point_ok = bi["point_ok"] & (truth >= 0)
    keep = bi["tri_inlier"] & point_ok[pt]
    pid = np.nonzero(point_ok)[0]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(pt[keep], minlength=len(pt_ptr) - 1)[pid])]).astype(np.int64)
    truth = truth[pid]
    ba = BundleAdjuster.from_observations(len(pid), 8, ptr, cam_idx[keep], xy[keep], X[pid], K, R, t, axis=bi["axis"], loss="huber",
                                          loss_scale=TC.E2E_DELTA)
    E0 = ba._engine.cost()
    ba.optimize()
    E = ba._engine.cost()
    E_gt = _huber_cost(len(pid), ptr, cam_idx[keep], xy[keep], sc.X_gt[truth], sc.K_gt, sc.R_gt, sc.t_gt, TC.E2E_DELTA)
    print(f"{len(pid)} points; huber cost {E0:.4e} -> {E:.4e}, ground truth {E_gt:.4e}")
    assert E < E_gt
