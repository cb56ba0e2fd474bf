"""The lane form's packed index row and its range count (csrc/mvba_engine_host.h: lane_idx_pack / lane_idx_unpack, lane_idx_fits,
lane_ranges), restated in NumPy and applied to the observation lists of tests/test_gpu_lanes_ranges.py alone: what every scene of
that file packs into, where its offsets l - k reach, and the number of point ranges mvba_create counts for it from three and from
four wave places per CU.  No GPU and no library: the restated rules are what the GPU tests assert schur_info() against."""
import numpy as np
import pytest

import _visibility_cases as V
from lib.synthetic import make_scene

ROW_BITS = 25                      # record index (from its range's first observation) and point row: 32-bit byte offsets of 128-byte rows
OFF_BITS = 2 * (32 - ROW_BITS)     # l - k, in the seven bits either word has left
ROW_MAX, OFF_MAX = (1 << ROW_BITS) - 1, (1 << OFF_BITS) - 1
MAX_RANGES = 64
CUS = 256                          # the MI355X


def pack(k, l, a):
    k, l, a = (np.asarray(v, np.int64) for v in (k, l, a))
    d = l - k
    return (k | (d & 127) << ROW_BITS).astype(np.uint32), (a | (d >> 7) << ROW_BITS).astype(np.uint32)


def unpack(w0, w1):
    w0, w1 = w0.astype(np.int64), w1.astype(np.int64)
    k = w0 & ROW_MAX
    return k, k + (w0 >> ROW_BITS) + ((w1 >> ROW_BITS) << 7), w1 & ROW_MAX


def fits(n, widest, max_degree):
    return n <= ROW_MAX and widest - 1 <= ROW_MAX and max_degree - 1 <= OFF_MAX


def lane_waves(pt_ptr, cam_idx, m):
    """Waves of 64 lists a point range needs (PairLists::slot_waves at W = 64) and the typical off-diagonal list."""
    target, S, _ = V.size_pair_lists(V.pair_counts(pt_ptr, cam_idx, m))
    return -(-int(np.trace(S)) // 64) + -(-int(S[np.triu_indices(m, 1)].sum()) // 64), target


def lane_ranges(places, waves, target, forced=0):
    if forced > 0:
        return min(forced, MAX_RANGES)
    cap = 8 * max(1, min(MAX_RANGES // 8, target // 512))
    return max(1, min(places // max(1, waves), cap))


def wide_case():
    """tests/test_gpu_compact_record.py::_wide_case: 1500 x 80 at 10 %, points 0, 700 and 1499 seen by all 80 cameras."""
    n, m = 1500, 80
    sc = make_scene(n, m, vis_p=1.0, project="numpy")
    keep = np.random.default_rng(V.SEED).random((n, m)) < 0.1
    keep[[0, 700, 1499]] = True
    keep[keep.sum(1) < 2, :2] = True
    return sc, V.masked(sc, keep)


def test_round_trip_at_the_edges_of_every_field():
    ks = np.array([0, 1, 127, 128, (1 << 24) + 5, ROW_MAX - OFF_MAX, ROW_MAX - 1, ROW_MAX])
    ds = np.array([0, 1, 63, 64, 79, 127, 128, 129, 255, 256, 8191, 8192, OFF_MAX - 1, OFF_MAX])
    as_ = np.array([0, 1, 77, 1 << 24, ROW_MAX - 1, ROW_MAX])
    k, d, a = (v.ravel() for v in np.meshgrid(ks, ds, as_, indexing="ij"))
    ok = k + d <= ROW_MAX
    k, d, a = k[ok], d[ok], a[ok]
    assert len(k) > 500 and (k + d).max() == ROW_MAX and d.max() == OFF_MAX and a.max() == ROW_MAX
    k2, l2, a2 = unpack(*pack(k, k + d, a))
    np.testing.assert_array_equal(k2, k), np.testing.assert_array_equal(l2, k + d), np.testing.assert_array_equal(a2, a)
    # the padding item (0, 0, N) is the point row alone; a diagonal item carries no offset; all three at their largest fill both words
    assert [int(w) for w in pack(0, 0, 1234567)] == [0, 1234567]
    assert [int(w) for w in pack(4711, 4711, 42)] == [4711, 42]
    assert [int(w) for w in pack(ROW_MAX - OFF_MAX, ROW_MAX, ROW_MAX)] == [(ROW_MAX - OFF_MAX) | 127 << 25, 0xFFFFFFFF]
    # one more than the offset field holds is lost off the top of w1: the guards, not the packing, keep such scenes out
    assert unpack(*pack(np.array([0]), np.array([OFF_MAX + 1]), np.array([0])))[1][0] == 0


def test_the_byte_offset_guards_imply_the_row_fields():
    """(N + 1) * 128 < 2^32 and (widest + 1) * 128 < 2^32, decide_schur_form's guards for the 32-bit gather offsets: the largest
    N (the padding row is row N) and the largest record index of a range they admit fit 25 bits; the degree bound is the packed
    row's own, 16,384 observations of one point."""
    n_max = (1 << 32) // 128 - 2
    assert (n_max + 1) * 128 < 1 << 32 <= (n_max + 2) * 128
    assert fits(n_max, n_max, OFF_MAX + 1) and not fits(n_max, n_max, OFF_MAX + 2)
    assert not fits(ROW_MAX + 1, 10, 2) and not fits(10, ROW_MAX + 2, 2) and fits(ROW_MAX, ROW_MAX + 1, 2)
    assert OFF_MAX + 1 == 16384


SCENES = {  # name: (n, m, p), waves per range, nR from three / four places per CU
    "2000x100": ((2000, 100, 0.1), 96, 8, 8),
    "3000x30": ((3000, 30, 0.3), 9, 8, 8),
    "4000x100": ((4000, 100, 0.1), 94, 8, 8),
}


@pytest.mark.parametrize("name", SCENES)
def test_the_gpu_scenes_pack_and_count_their_ranges(name):
    """Small scenes: the typical list has fewer than 1024 items, so the cap is 8 ranges whatever the places -- the GPU tests
    force 1, 3, 10 and 11 with MVBA_SLOT_RANGES, and 11 x 96 waves are more than the chip's 1024 places."""
    (n, m, p), waves, nr3, nr4 = SCENES[name]
    sc = make_scene(n, m, vis_p=p)
    w, target = lane_waves(sc.pt_ptr, sc.cam_idx, m)
    deg = np.diff(sc.pt_ptr)
    assert w == waves <= 96 and target < 1024
    assert fits(n, sc.n_obs, int(deg.max())) and deg.max() - 1 < 128
    assert (lane_ranges(3 * CUS, w, target), lane_ranges(4 * CUS, w, target)) == (nr3, nr4)
    assert [lane_ranges(4 * CUS, w, target, f) for f in (1, 3, 10, 11, 64, 65)] == [1, 3, 10, 11, 64, 64]
    assert name != "2000x100" or 11 * w > 4 * CUS >= 10 * w


def test_the_flagship_plan():
    """1 M x 100 x 10 % (bench.py's config 3: ~95 waves per range, ~10,000 items in the typical list) from the rule alone: 8
    ranges at three places per CU -- the plan before the packed row --, 10 at four; 90 and 80 cameras: 13 and 16."""
    assert lane_ranges(3 * CUS, 95, 10000) == 8 and lane_ranges(4 * CUS, 95, 10000) == 10
    assert lane_ranges(4 * CUS, 78, 10000) == 13 and lane_ranges(4 * CUS, 63, 10000) == 16
    assert lane_ranges(4 * CUS, 96, 10000) == 10 and lane_ranges(1000, 96, 10000) == 10 and lane_ranges(959, 96, 10000) == 9
    assert lane_ranges(4 * CUS, 2000, 10000) == 1 and lane_ranges(4 * CUS, 1, 1 << 40) == MAX_RANGES


def test_a_scene_whose_ranges_follow_the_places():
    """110,000 x 100 x 10 %: the typical list has 1024 items or more, the cap is 16, and the count is the places' -- 8 from three
    per CU, 10 from four (what tests/test_gpu_lanes_ranges.py asserts of the plan mvba_create makes by itself)."""
    sc = make_scene(110000, 100, vis_p=0.1)
    w, target = lane_waves(sc.pt_ptr, sc.cam_idx, 100)
    assert 1024 <= target < 1536 and 86 <= w <= 96
    assert (lane_ranges(3 * CUS, w, target), lane_ranges(4 * CUS, w, target)) == (8, 10)


def test_the_wide_case_reaches_offsets_past_64():
    """Points seen by all 80 cameras: offsets up to 79 (seven bits; the low field is full from 127 on).  Without a camera twice in
    a point an offset stays below the camera count, and the lane form's 96 waves of 64 lists admit ~110 cameras: the high field
    is reached by no scene the GPU tests can build -- its round trip is the test above and csrc/host_check.cpp."""
    sc, (pt_ptr, cam_idx, _) = wide_case()
    deg = np.diff(pt_ptr)
    assert deg.max() == 80 and (deg == 80).sum() == 3
    w, _ = lane_waves(pt_ptr, cam_idx, 80)
    assert w <= 96 and fits(sc.n_points, len(cam_idx), 80)
    o = pt_ptr[700] + np.array([0, 64, 79])
    k2, l2, a2 = unpack(*pack(np.full(3, o[0]), o, np.full(3, 700)))
    assert (l2 - k2).tolist() == [0, 64, 79] and (a2 == 700).all()
