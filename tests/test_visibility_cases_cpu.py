"""The structured visibility families of tests/_visibility_cases.py reach the regimes of csrc/mvba_create.h they are named
for -- shown on the host from the case's observation list and the sizing formulas alone -- and the oracle's damped reduced
system on them is positive definite (a GPU test that ended in the LU rescue would say nothing about K3)."""
import numpy as np
import pytest

import _visibility_cases as V

C = 1e-2  # the damping at which the forms of K3 are compared with the oracle (test_gpu_parity.py)

# per case, all exact: (empty, all) off-diagonal camera pairs, (min, max) point degree, (min, max) camera degree
EXPECT = {
    "band_3000x14": dict(empty=(55, 91), deg=(2, 4), cam_deg=(95, 841)),
    "band_30000x24": dict(empty=(210, 276), deg=(2, 4), cam_deg=(485, 4372)),
    "hub_20000x40": dict(empty=(0, 780), deg=(2, 40), cam_deg=(463, 20000)),
    "blocks_20000x20": dict(empty=(0, 190), deg=(2, 20), cam_deg=(4929, 5118)),
    "heavy_1500x60": dict(empty=(0, 1770), deg=(2, 60), cam_deg=(27, 54)),
    "band_150000x34": dict(empty=(465, 561), deg=(2, 4), cam_deg=(1651, 14626)),
}


@pytest.fixture(scope="module", params=list(V.CASES))
def plan(request):
    name = request.param
    sc, pt_ptr, cam_idx, xy = V.case(name)
    m = sc.n_images
    cnt = V.pair_counts(pt_ptr, cam_idx, m)
    target, S, slot_waves = V.size_pair_lists(cnt)
    return dict(name=name, n=sc.n_points, m=m, pt_ptr=pt_ptr, cam_idx=cam_idx, xy=xy, cnt=cnt, target=target, S=S,
                slot_waves=slot_waves, lo=V.slot_ranges(pt_ptr, target, slot_waves))


def test_case_is_a_masked_make_scene(plan):
    """The observation list is well formed (ascending distinct cameras inside a point), its coordinates are make_scene's, and
    the pair counts restated here add up to sum d (d + 1) / 2."""
    sc = V.case(plan["name"])[0]
    n, m, pt_ptr, cam = plan["n"], plan["m"], plan["pt_ptr"], plan["cam_idx"]
    assert pt_ptr[0] == 0 and pt_ptr[-1] == len(cam) == len(plan["xy"]) and len(pt_ptr) == n + 1
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    inside = pt[1:] == pt[:-1]
    assert (np.diff(cam.astype(np.int64))[inside] > 0).all() and cam.min() == 0 and cam.max() == m - 1
    np.testing.assert_array_equal(plan["xy"], sc.xy.reshape(n, m, 2)[pt, cam])
    d = np.diff(pt_ptr)
    assert plan["cnt"][np.triu_indices(m)].sum() == (d * (d + 1) // 2).sum()
    np.testing.assert_array_equal(np.diag(plan["cnt"]), np.bincount(cam, minlength=m))


def test_degrees_and_empty_pairs(plan):
    e = EXPECT[plan["name"]]
    m = plan["m"]
    off = np.triu_indices(m, 1)
    assert (int((plan["cnt"][off] == 0).sum()), len(off[0])) == e["empty"]
    d = np.diff(plan["pt_ptr"])
    assert (d.min(), d.max()) == e["deg"]
    cd = np.bincount(plan["cam_idx"], minlength=m)
    assert (cd.min(), cd.max()) == e["cam_deg"]  # (min > 0: a camera without observations is singular by construction)
    assert plan["slot_waves"] <= 32 * 9  # MVBA_SCHUR=slots is honoured: all lists of a range fit one XCD


@pytest.mark.parametrize("name", [k for k in V.CASES if k.startswith("band")])
def test_band_lists_are_confined_to_a_stretch_of_the_sweep(name):
    """band: no camera's points span more than (w + 1) / (m - w + 1) of the sweep -- so neither does any pair's list -- and
    the cameras' degrees differ severalfold (queues and waves of unequal length)."""
    sc, pt_ptr, cam, _ = V.case(name)
    n, m = sc.n_points, sc.n_images
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    first, last = np.full(m, n), np.full(m, -1)
    np.minimum.at(first, cam, pt)
    np.maximum.at(last, cam, pt)
    assert (last - first).max() <= n * (V.BAND_W + 1) // (m - V.BAND_W + 1)
    cd = np.bincount(cam, minlength=m)
    assert cd.max() >= 4 * cd.min()


def test_hub_reaches_the_sublist_cap_and_a_small_target():
    sc, pt_ptr, cam_idx, _ = V.case("hub_20000x40")
    cnt = V.pair_counts(pt_ptr, cam_idx, 40)
    target, S, _ = V.size_pair_lists(cnt)
    assert 16 <= target <= 64  # "a few dozen"
    assert S.max() == V.S_CAP == S[0, 0] and (cnt[0, 0] + target // 2) // target > V.S_CAP  # the clamp is what holds it
    cd = np.bincount(cam_idx, minlength=40)
    assert cd[0] == 20000 and cd[1:].max() < 2 * 20000 // 39 + 8  # camera degree n next to ~n / m
    d = np.diff(pt_ptr)
    assert (d == 40).sum() == 8 and (d == 2).sum() == 20000 - 8


def test_blocks_lists_are_absent_from_half_the_ranges():
    """blocks: a pair inside a cluster has no item in the other cluster's point ranges (the bridge points sit in the two
    ranges around n / 2), so its list is absent from at least nR / 2 - 1 of the slot form's ranges; a pair across the
    clusters holds the 20 bridge points only and is absent from all ranges but those two."""
    sc, pt_ptr, cam_idx, _ = V.case("blocks_20000x20")
    m = 20
    cnt = V.pair_counts(pt_ptr, cam_idx, m)
    target, S, sw = V.size_pair_lists(cnt)
    lo = V.slot_ranges(pt_ptr, target, sw)
    nR = len(lo) - 1
    assert nR >= 8
    assert (cnt[:10, 10:] == 20).all() and cnt[:10, :10][np.triu_indices(10, 1)].min() > 1000
    present = np.stack([V.pair_counts(pt_ptr[lo[r]:lo[r + 1] + 1] - pt_ptr[lo[r]], cam_idx[pt_ptr[lo[r]]:pt_ptr[lo[r + 1]]], m) > 0
                        for r in range(nR)])  # (nR, m, m)
    absent = nR - present.sum(0)
    iu = np.triu_indices(10)
    assert absent[:10, :10][iu].min() >= nR // 2 - 1 and absent[10:, 10:][iu].min() >= nR // 2 - 1
    assert absent[:10, 10:].min() >= nR - 2
    # whole waves: 21 consecutive off-diagonal lists of the second cluster's cameras have no item in the first ranges
    assert not present[:nR // 2 - 1, 10:, 10:].any()


def test_heavy_leaves_point_ranges_empty():
    sc, pt_ptr, cam_idx, _ = V.case("heavy_1500x60")
    cnt = V.pair_counts(pt_ptr, cam_idx, 60)
    target, S, sw = V.size_pair_lists(cnt)
    assert target < 16  # a `target` of a few items
    lo = V.slot_ranges(pt_ptr, target, sw)
    assert len(lo) == 9  # 8 ranges
    assert (np.diff(lo) == 0).sum() >= 1 and (np.diff(lo) < 0).sum() == 0
    assert [int(v) for v in lo[1:3]] == [301, 301] and [int(v) for v in lo[7:]] == [1500, 1500]


def test_skew_scene_has_wide_ranges_and_lists_that_start_far_apart():
    """The skew-idling scene: 8 ranges, each wider than 2 x SLOT_SKEW observations, and inside one range two non-empty pairs
    (k, l), (k, l + 1) -- neighbours in a wave -- whose first items lie more than SLOT_SKEW observations apart."""
    sc, pt_ptr, cam_idx, _ = V.case(V.SKEW_CASE)
    assert V.skew_precondition(pt_ptr, cam_idx, sc.n_images)


def test_oracle_system_is_positive_definite(plan):
    g = V.oracle_for(plan["name"])
    g.linearize()
    E0 = g.cost()
    E1 = g.try_step(C)
    w = np.linalg.eigvalsh(g.A)
    assert w.min() > 0 and w.max() / w.min() < 1e7, (w.min(), w.max())
    assert np.isfinite(E1) and E1 < E0
