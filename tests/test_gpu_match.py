"""Descriptor matching on the device: mvba_match_descriptors against the NumPy reference (tests/_match_ref.py) on
the cases of tests/_match_cases.py and on the limit cases beside them -- every comparison exact --, its independence of the rest of the pair list, its
repeatability, and a scene's descriptors through match_descriptors, verify_matches, build_tracks, bootstrap and Huber bundle
adjustment."""
import numpy as np
import pytest

from lib import _mvba
from lib.bundle_adjustment import BundleAdjuster
from lib.initialization import bootstrap, build_tracks, match_descriptors, verify_matches

import _match_cases as MC
import _match_ref as MR
import _tracks_cases as TRC

pytestmark = pytest.mark.gpu

ARRAYS = ("match_ptr", "kp_pairs", "dist2", "nn_best", "nn_dist2", "nn_second2")


def _run(name, pairs=None, case=MC.case):
    kp_ptr, desc, all_pairs, kw = case(name)
    kw = dict(kw, ratio=0.0 if kw["ratio"] is None else kw["ratio"])
    return _mvba.match_descriptors(kp_ptr, desc, all_pairs if pairs is None else pairs, want_nn=True, **kw)


def _same(got, want, what):
    for key in ARRAYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
        assert got[key].tobytes() == want[key].tobytes(), (what, key, np.nonzero(got[key].reshape(-1) != want[key].reshape(-1))[0][:8])
    for key in MR.COUNTS:
        assert got[key] == want[key], (what, key, got[key], want[key])


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_case_matches_the_reference(name):
    got = _run(name)
    print(f"{name}: {got['n_matches']} matches of {got['n_queries']} queries, timings {got['timings_ms']}")
    _same(got, MC.reference(name), name)
    if name == "orientation":
        np.testing.assert_array_equal(got["nn_best"], MC.orientation_perm())
    if name == "index_width":
        assert got["nn_best"].tolist() == list(MC.WIDTH_BEST)
    if name == "flat":
        assert (got["nn_dist2"] == MC.FLAT_D2).all() and (got["nn_second2"] == MC.FLAT_D2).all() and (got["nn_best"] == 0).all()
    # without the per-query arrays: the same matches
    kp_ptr, desc, pairs, kw = MC.case(name)
    bare = _mvba.match_descriptors(kp_ptr, desc, pairs, **dict(kw, ratio=kw["ratio"] or 0.0))
    assert "nn_best" not in bare and all(bare[k].tobytes() == got[k].tobytes() for k in ARRAYS[:3])


@pytest.mark.parametrize("name", sorted(MC.LIMIT_CASES))
def test_limit_case_matches_the_reference(name):
    """The limits pass of DESIGN.md §25: every k-step count at its edges, the flat extremes per instantiation, ties and
    orderings by the candidates' places in the wave, the wave edges of a query block, and more query rows than the scan's
    second level takes in one trip.  What each case is for is asserted on the reference alone in tests/test_match_cpu.py."""
    got = _run(name, case=MC.limit_case)
    print(f"{name}: {got['n_matches']} matches of {got['n_queries']} queries, timings {got['timings_ms']}")
    want = MC.limit_reference(name)
    _same(got, want, name)
    if name.startswith("flat"):
        d = int(name[-3:])
        assert (got["nn_second2"][:40] == d * 255 ** 2).all()
        if name.startswith("flat_one"):
            assert (got["nn_best"][:40] == 17).all() and (got["nn_dist2"][:40] == d * 255 ** 2 - 255 ** 2 + 254 ** 2).all()
        else:
            assert (got["nn_best"] == 0).all() and (got["nn_dist2"] == d * 255 ** 2).all() and (got["nn_second2"] == d * 255 ** 2).all()
    if name == "ties":
        for variant, rows, q, best, best2, second2 in MC.ties()[1]:
            assert (got["nn_best"][q], got["nn_dist2"][q], got["nn_second2"][q]) == (best, best2, second2), (variant, rows, MC.lane_of_row(rows[0]),
                                                                                                             MC.lane_of_row(rows[1]))
    if name.startswith("scan258"):
        assert got["match_ptr"][1] == got["match_ptr"][2] and got["match_ptr"][4] == got["match_ptr"][3] + 1  # the empty image; the last query
        assert got["kp_pairs"][-1].tolist() == [0, 2] and got["dist2"][-1] == 1


def test_a_pair_is_answered_whatever_the_rest_of_the_list():
    """Every pair of the tile-edge case asked alone gives its part of the answer to the whole list; the list reversed, with one
    pair doubled, gives the parts in that order."""
    kp_ptr, _, pairs, _ = MC.case("tiles")
    whole = _run("tiles")
    qptr = np.concatenate([[0], np.cumsum(np.diff(kp_ptr)[pairs[:, 0]])])
    mptr = whole["match_ptr"]

    def part(i):
        return {"kp_pairs": whole["kp_pairs"][mptr[i]:mptr[i + 1]], "dist2": whole["dist2"][mptr[i]:mptr[i + 1]],
                **{k: whole[k][qptr[i]:qptr[i + 1]] for k in ARRAYS[3:]}}
    for i in range(len(pairs)):
        alone = _run("tiles", pairs[i:i + 1])
        assert alone["match_ptr"].tolist() == [0, mptr[i + 1] - mptr[i]]
        for key, want in part(i).items():
            assert alone[key].tobytes() == want.tobytes(), (i, key)
    order = list(range(len(pairs)))[::-1] + [7]
    turned = _run("tiles", pairs[order])
    np.testing.assert_array_equal(np.diff(turned["match_ptr"]), np.diff(mptr)[order])
    for key in ("kp_pairs", "dist2") + ARRAYS[3:]:
        assert turned[key].tobytes() == np.concatenate([part(i)[key] for i in order]).tobytes(), key


@pytest.mark.parametrize("name", MC.LARGEST)
def test_two_calls_are_bitwise_equal(name):
    a, b = _run(name), _run(name)
    for key in ARRAYS:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert all(a[k] == b[k] for k in MR.COUNTS)


def test_a_long_pair_list_is_cut_into_chunks():
    """The index-width pair asked CHUNK_PAIRS times in one call (the ABI answers a duplicate as often as it is listed): more
    query rows than a chunk holds, so the list is cut, and every copy gets the single pair's answer at its own place."""
    kp_ptr, desc, pairs, kw = MC.case("index_width")
    assert MC.CHUNK_PAIRS * int(kp_ptr[-1]) > MC.CHUNK_ROWS > 2 * int(kp_ptr[-1])  # cut inside the list, several pairs to a chunk
    one = MC.reference("index_width")
    got = _run("index_width", np.tile(pairs, (MC.CHUNK_PAIRS, 1)))
    np.testing.assert_array_equal(got["match_ptr"], one["match_ptr"][1] * np.arange(MC.CHUNK_PAIRS + 1))
    for key in ARRAYS[1:]:
        assert got[key].tobytes() == np.concatenate([one[key]] * MC.CHUNK_PAIRS).tobytes(), key
    assert all(got[k] == MC.CHUNK_PAIRS * one[k] for k in MR.COUNTS)


def test_python_form_returns_the_reference():
    kp_ptr, desc, pairs, kw = MC.case("rules")
    ref = MC.reference("rules")
    matches, info = match_descriptors((kp_ptr, desc), pairs, ratio=kw["ratio"], mutual=kw["mutual"], max_distance=MC.RULES_MAX_DISTANCE,
                                      return_nn=True)
    assert list(matches) == [tuple(p) for p in pairs.tolist()] == list(info["distance2"]) == list(info["nn_best"])
    qptr = np.concatenate([[0], np.cumsum(np.diff(kp_ptr)[pairs[:, 0]])])
    for i, kl in enumerate(matches):
        m = slice(ref["match_ptr"][i], ref["match_ptr"][i + 1])
        assert matches[kl].dtype == np.int64
        np.testing.assert_array_equal(matches[kl], ref["kp_pairs"][m])
        np.testing.assert_array_equal(info["distance2"][kl], ref["dist2"][m])
        for mine, theirs in (("nn_best", "nn_best"), ("nn_distance2", "nn_dist2"), ("nn_second2", "nn_second2")):
            np.testing.assert_array_equal(info[mine][kl], ref[theirs][qptr[i]:qptr[i + 1]])
    assert all(info[k] == ref[k] for k in MR.COUNTS)
    arrays = [desc[kp_ptr[i]:kp_ptr[i + 1]] for i in range(4)]  # a list of arrays, every k < l
    every, _ = match_descriptors(arrays, ratio=None, mutual=False)
    assert list(every) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] and len(every[(0, 1)]) == 40 and len(every[(0, 2)]) == 0


def _huber_cost(n, pt_ptr, cam, xy, X, K, R, t, delta):
    eng = _mvba.HipEngine(n, 8, pt_ptr, cam, xy, 1.0, "x-up_z-forward", loss="huber", loss_scale=delta)
    eng.set_params(X, K[:, 0, 0], K[:, :2, 2], t, R)
    E = eng.cost()
    eng.close()
    return E


def test_descriptors_to_bundle_adjustment():
    """The scene's descriptors, with 20 points that look like 20 others: matched at ratio 0.8 over all 28 pairs -- exactly the
    reference's matches --, verified pair by pair, built into tracks, bootstrapped with the three robust thresholds and
    bundle-adjusted under the Huber loss.  All 8 cameras are registered and the final cost is below that of the ground truth
    on the same list (the premise is tests/test_match_cpu.py::test_premise_of_the_end_to_end_case)."""
    sc, sd = TRC.scene(), MC.scene_descriptors()
    mo = sd.mo
    matches, mi = match_descriptors(sd.descriptors, ratio=MC.E2E_RATIO)
    want = MC.scene_reference(MC.E2E_RATIO)
    assert list(matches) == list(want)
    for kl in want:
        np.testing.assert_array_equal(matches[kl], want[kl])
    true, twins, other, n_true = MC.scene_score(matches)
    ok, vi = verify_matches(mo.keypoints, matches, TRC.E2E_THRESHOLD, n_hypotheses=TRC.E2E_HYP, seed=TRC.E2E_SEED)
    true_v, twins_v, other_v, _ = MC.scene_score({kl: matches[kl][ok[kl]] for kl in matches})
    pt_ptr, cam_idx, xy, info = build_tracks(mo.keypoints, matches, match_ok=ok)
    share = TRC.foreign_share(mo, cam_idx, info["kp_idx"], pt_ptr)
    print(f"{mi['n_matches']} matches: {true} true of {n_true}, {twins} between twins, {other} other wrong; verified: {true_v} true, "
          f"{twins_v + other_v} wrong; tracks {info['n_tracks']}, foreign share {share:.4f}; timings {mi['timings_ms']}")
    thr = TRC.E2E_THRESHOLD
    K, R, t, X, bi = bootstrap(pt_ptr, cam_idx, xy, sc.init_K, ransac_threshold=thr, pose_threshold=thr, triangulate_threshold=thr,
                               n_hypotheses=TRC.E2E_HYP, seed=TRC.E2E_SEED)
    assert bi["camera_ok"].all() and len(bi["order"]) == 8
    truth = TRC.track_points(mo, cam_idx, info["kp_idx"], pt_ptr)[0]
    pt = np.repeat(np.arange(len(pt_ptr) - 1), np.diff(pt_ptr))
    point_ok = bi["point_ok"] & (truth >= 0)
    keep = bi["tri_inlier"] & point_ok[pt]
    pid = np.nonzero(point_ok)[0]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(pt[keep], minlength=len(pt_ptr) - 1)[pid])]).astype(np.int64)
    truth = truth[pid]
    ba = BundleAdjuster.from_observations(len(pid), 8, ptr, cam_idx[keep], xy[keep], X[pid], K, R, t, axis=bi["axis"], loss="huber",
                                          loss_scale=TRC.E2E_DELTA)
    E0 = ba._engine.cost()
    ba.optimize()
    E = ba._engine.cost()
    E_gt = _huber_cost(len(pid), ptr, cam_idx[keep], xy[keep], sc.X_gt[truth], sc.K_gt, sc.R_gt, sc.t_gt, TRC.E2E_DELTA)
    print(f"{len(pid)} points; huber cost {E0:.4e} -> {E:.4e}, ground truth {E_gt:.4e}")
    assert E < E_gt
