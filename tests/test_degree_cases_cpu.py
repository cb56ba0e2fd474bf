"""The degree families of tests/_degree_cases.py reach the code they are named for -- K1's split tiles in every layout, every
(lanes, block) cell of K5, k_point_cov at eight lanes on points of thousands of pairs -- shown on the host from the case's
observation list and the restated rules of csrc/mvba_create.h and csrc/mvba.hip (the launch side) alone; the oracle's damped reduced system on
them is positive definite; and the figures the GPU margins of tests/test_gpu_degree.py are 100 x of are re-measured here."""
import numpy as np
import pytest

import _degree_cases as D
import _visibility_cases as V

C = 1e-2  # the damping at which tests/test_gpu_degree.py compares with the oracle

# per case, all exact: (min, max) point degree, (min, max) camera degree, observations, (tiles, split tiles) of K1
EXPECT = {
    "tall_1500x80": dict(deg=(2, 80), cam_deg=(10, 83), n_obs=5716, tiles=(97, 10)),
    "tall_2000x130": dict(deg=(2, 130), cam_deg=(8, 62), n_obs=6731, tiles=(112, 14)),
    "tall_6000x300": dict(deg=(3, 300), cam_deg=(9, 84), n_obs=22102, tiles=(358, 21)),
    "wide_40x110": dict(deg=(110, 110), cam_deg=(40, 40), n_obs=4400, tiles=(80, 80)),
    "wide_60x200_60": dict(deg=(106, 140), cam_deg=(18, 47), n_obs=7133, tiles=(124, 124)),
    "wide_60x400_35": dict(deg=(105, 164), cam_deg=(11, 33), n_obs=8396, tiles=(174, 174)),
    "wide_80x647_20": dict(deg=(109, 160), cam_deg=(6, 28), n_obs=10241, tiles=(199, 199)),
    "wide_60x200_35": dict(deg=(50, 87), cam_deg=(10, 33), n_obs=4239, tiles=(108, 96)),
    "wide_80x400_20": dict(deg=(59, 98), cam_deg=(7, 26), n_obs=6316, tiles=(159, 158)),
    "wide_200x647_10": dict(deg=(42, 81), cam_deg=(8, 33), n_obs=12662, tiles=(285, 170)),
}


def _lists(name):
    sc, pt_ptr, cam_idx, xy = D.case(name)
    return sc.n_points, sc.n_images, pt_ptr, cam_idx, xy


# ---------------------------------------------------------------- 3 (first: the others build on a well-formed list)
@pytest.mark.parametrize("name", D.CASES)
def test_case_is_a_masked_make_scene_with_the_stated_degrees(name):
    """Ascending distinct cameras inside a point, make_scene's coordinates, the exact degree extremes, and every camera with
    at least MIN_CAMERA_DEGREE observations (the covariance inverts the UNDAMPED reduced system)."""
    sc = D.case(name)[0]
    n, m, pt_ptr, cam, xy = _lists(name)
    assert pt_ptr[0] == 0 and pt_ptr[-1] == len(cam) == len(xy) and len(pt_ptr) == n + 1
    pt = np.repeat(np.arange(n), np.diff(pt_ptr))
    assert (np.diff(cam.astype(np.int64))[pt[1:] == pt[:-1]] > 0).all() and cam.min() == 0 and cam.max() == m - 1
    np.testing.assert_array_equal(xy, sc.xy.reshape(n, m, 2)[pt, cam])
    assert not xy.flags.writeable and not pt_ptr.flags.writeable and not cam.flags.writeable
    e = EXPECT[name]
    d, cd = np.diff(pt_ptr), np.bincount(cam, minlength=m)
    assert (int(d.min()), int(d.max())) == e["deg"] and (int(cd.min()), int(cd.max())) == e["cam_deg"] and len(cam) == e["n_obs"]
    assert cd.min() >= D.MIN_CAMERA_DEGREE
    if name in D.TALL:
        for a, deg in D.TALL[name][2].items():
            assert d[a] == deg and cam[pt_ptr[a]:pt_ptr[a + 1]].tolist() == list(range(deg))
        short = np.delete(d, list(D.TALL[name][2]))
        assert (short.max(), short.min()) == D.TALL[name][3:]


# ---------------------------------------------------------------- 1: the tile layout
def _layout(pt_ptr):
    tiles, tile_slot, splits = D.k1_tiles(pt_ptr)
    o0, o1, split = D.tile_ranges(tiles)
    return tiles, tile_slot, splits, o0, o1, split


@pytest.mark.parametrize("name", D.CASES)
def test_tiles_cover_the_observations_and_pieces_tile_their_point(name):
    """The restated build_k1_tiles: the tiles partition [0, n_obs) into runs of 1 .. 64, a packed tile holds whole points, a
    split tile one piece of one point of more than 64, the pieces of every split point tile its range exactly in slot order,
    and tile_slot is -1 exactly at the packed tiles and the terminator."""
    n, m, pt_ptr, cam, _ = _lists(name)
    tiles, tile_slot, splits, o0, o1, split = _layout(pt_ptr)
    assert (len(tiles) - 1, int(split.sum())) == EXPECT[name]["tiles"]
    assert o0[0] == 0 and o1[-1] == pt_ptr[-1] == tiles[-1] and (o0[1:] == o1[:-1]).all()
    assert ((o1 - o0) >= 1).all() and ((o1 - o0) <= 64).all()
    d = np.diff(pt_ptr)
    starts = set(pt_ptr.tolist())
    for t in np.nonzero(~split)[0]:  # whole points of at most 64
        assert int(o0[t]) in starts and int(o1[t]) in starts
        a0, a1 = np.searchsorted(pt_ptr, [o0[t], o1[t]])
        assert d[a0:a1].max() <= 64
    assert (tile_slot[:-1][~split] == -1).all() and tile_slot[-1] == -1
    assert tile_slot[:-1][split].tolist() == list(range(int(split.sum())))  # slots in tile order
    assert splits[:, 0].tolist() == np.nonzero(d > 64)[0].tolist()
    slot_tile = np.nonzero(split)[0]
    for a, s0, pieces in splits.tolist():
        assert pieces == -(-d[a] // 64) >= 2
        ts = slot_tile[s0:s0 + pieces]
        assert (np.diff(ts) == 1).all()  # consecutive tiles
        assert o0[ts[0]] == pt_ptr[a] and o1[ts[-1]] == pt_ptr[a + 1]
        assert ((o1 - o0)[ts[:-1]] == 64).all() and (o1 - o0)[ts[-1]] == d[a] - 64 * (pieces - 1)
    assert splits[:, 2].sum() == split.sum()


def layout_features(pt_ptr):
    """The features of a tile layout that K1, tile_slot and k_sum_split have to get right, from the observation list."""
    tiles, tile_slot, splits, o0, o1, split = _layout(pt_ptr)
    d = np.diff(pt_ptr)
    last_piece = d[splits[:, 0]] - 64 * (splits[:, 2] - 1)
    inner = tile_slot[:-1]
    first, last = np.nonzero(inner >= 0)[0][[0, -1]] if split.any() else (0, -1)
    return dict(
        any_split=bool(split.any()),
        packed_then_split=bool((~split[:-1] & split[1:]).any()),  # tile_start[t + 1] complemented, tile_start[t] not
        split_then_packed=bool((split[:-1] & ~split[1:]).any()),  # ... and the reverse
        first_tile_split=bool(tiles[0] == -1),                    # ~0
        terminator_after_split=bool(split[-1]),
        pieces=sorted(set(splits[:, 2].tolist())),
        last_piece_of_one=bool((last_piece == 1).any()),
        last_piece_full=bool((last_piece == 64).any()),
        degrees=set(d[d >= 64].tolist()),
        slot_gaps=bool(split.any() and (inner[first:last + 1] == -1).any()),  # -1 entries between two slots
        two_splits_in_a_row=bool((np.diff(splits[:, 0]) == 1).any()),
        part_filled_packed_tile=bool((~split & ((o1 - o0) < 64 - 4)).any()),
        point_of_64_alone=bool((~split & ((o1 - o0) == 64) & np.isin(o0, pt_ptr[:-1][d == 64])).any()),
    )


TALL_FEATURES = {
    "tall_1500x80": dict(pieces=[2], degrees={64, 65, 66, 79, 80}),
    "tall_2000x130": dict(pieces=[2, 3], degrees={64, 65, 66, 127, 128, 129, 130}),
    "tall_6000x300": dict(pieces=[2, 3, 4, 5], degrees={64, 65, 128, 129, 193, 257, 300}),
}


@pytest.mark.parametrize("name", list(D.TALL))
def test_tall_cases_have_every_layout_feature(name):
    f = layout_features(D.case(name)[1])
    for key in ("any_split", "packed_then_split", "split_then_packed", "first_tile_split", "terminator_after_split",
                "last_piece_of_one", "slot_gaps", "two_splits_in_a_row", "part_filled_packed_tile", "point_of_64_alone"):
        assert f[key], key
    assert f["pieces"] == TALL_FEATURES[name]["pieces"] and f["degrees"] == TALL_FEATURES[name]["degrees"]
    if name != "tall_1500x80":
        assert f["last_piece_full"] and {64, 128, 129} <= f["degrees"] and 3 in f["pieces"]
    # k_sum_split over points with different piece counts: from three pieces up
    assert name == "tall_1500x80" or len(f["pieces"]) >= 2
    # the packed tile of points 1 .. 6, the point of exactly 64 alone, then two split points
    pt_ptr = D.case(name)[1]
    tiles, _, _, o0, o1, split = _layout(pt_ptr)
    t = int(np.nonzero(o0 == pt_ptr[1])[0][0])
    assert not split[t] and o1[t] == pt_ptr[7] and not split[t + 1] and (o0[t + 1], o1[t + 1]) == (pt_ptr[7], pt_ptr[8])
    assert split[t + 2] and o0[t + 2] == pt_ptr[8]


def test_the_mixed_wide_case_splits_part_of_its_points():
    f = layout_features(D.case("wide_200x647_10")[1])
    assert f["packed_then_split"] and f["split_then_packed"] and f["pieces"] == [2] and f["slot_gaps"]
    d = np.diff(D.case("wide_200x647_10")[1])
    assert ((d > 64).sum(), (d <= 64).sum()) == (85, 115)


def test_layout_premises_bite():
    """A copy of a tall case in which no point exceeds 64 observations has no split tile, and none of the features."""
    n, m, tall, w, w_min = D.TALL["tall_2000x130"]
    keep = D.tall_mask(n, m, {a: min(d, 64) for a, d in tall.items()}, w, w_min)
    pt_ptr = np.concatenate([[0], np.cumsum(keep.sum(1))])
    f = layout_features(pt_ptr)
    assert not f["any_split"] and not f["packed_then_split"] and not f["first_tile_split"] and not f["terminator_after_split"]
    assert f["pieces"] == [] and not f["slot_gaps"] and not f["last_piece_of_one"]
    assert D.k1_tiles(pt_ptr)[2].shape == (0, 3)


# ---------------------------------------------------------------- 2: the width rules
def _cells(cell=D.k5_cell):
    out = {}
    for name in D.CASES:
        n, m, pt_ptr, cam, _ = _lists(name)
        out[name] = cell(len(cam), n, m)
    return out


def test_every_case_reaches_its_k5_cell_and_covariance_width():
    assert _cells() == D.K5_CELL
    for name in D.TALL:
        n, m, pt_ptr, cam, _ = _lists(name)
        assert D.cov_lanes(len(cam), n) == 8
    assert D.cov_lanes(4400, 40) == 64  # wide_40x110
    # the camera counts sit where the issue puts them: 256 threads up to 182 cameras, 512 up to 365, 1024 up to 646
    assert [D.k5_cell(10, 1, m)[1] for m in (182, 183, 365, 366, 646, 647)] == [256, 512, 512, 1024, 1024, D.GCAM]


def test_robust_only_scenes_reach_their_k5_cells_and_leave_every_camera_enough():
    """The scenes of ROBUST_WIDE, from their observation lists: the (G, bt) cell of k_backsub each is there for, and every
    camera with MIN_CAMERA_DEGREE observations.  With them ROBUST_CASES and the two cells of tests/test_gpu_robust.py cover
    all twelve."""
    for name, cell in D.ROBUST_WIDE_K5_CELL.items():
        n, m, pt_ptr, cam, _ = _lists(name)
        assert (n, m) == D.ROBUST_WIDE[name][:2] and D.k5_cell(len(cam), n, m) == cell, name
        assert np.bincount(cam, minlength=m).min() >= D.MIN_CAMERA_DEGREE, name
    assert set(D.ROBUST_WIDE_K5_CELL) == set(D.ROBUST_WIDE) and not set(D.ROBUST_WIDE) & set(D.CASES)
    cells = {{**D.K5_CELL, **D.ROBUST_WIDE_K5_CELL}[name] for name in D.ROBUST_CASES}
    assert cells | {(2, 256), (2, D.GCAM)} == D.ALL_K5_CELLS


def test_mean_degrees_are_five_percent_clear_of_every_threshold():
    """n_obs / N is formed in double on the device side too; 5 % is far beyond any rounding of it."""
    for name in D.CASES:
        n, m, pt_ptr, cam, _ = _lists(name)
        deg = len(cam) / n
        for lim in D.K5_G_LIMITS:
            assert abs(deg - lim) >= 0.05 * lim, (name, deg, lim)
        pairs = 0.5 * deg * (deg + 1.0)
        for lim in D.COV_G_LIMITS:
            assert abs(pairs - lim) >= 0.05 * lim, (name, pairs, lim)


def _old_cells(cell=D.k5_cell):
    return {cell(round(n * m * p), n, m) for n, m, p in D.OLD_K5_SCENES}


def test_the_cases_and_the_older_scenes_cover_all_twelve_k5_cells():
    """With (90, 70, 1.0), the only older scene at four lanes, these cases cover the four- and eight-lane columns entirely and
    two lanes at 256 and 512 threads; two lanes at 1024 threads and with GCAM are the 646- and 647-camera scenes of
    tests/test_gpu_parity.py."""
    assert D.k5_cell(90 * 70, 90, 70) == (4, 256) and _old_cells() == {(4, 256), (2, 1024), (2, D.GCAM)}
    new = set(_cells().values())
    assert new | {(4, 256)} >= {(G, bt) for G in (4, 8) for bt in (256, 512, 1024, D.GCAM)}
    assert new | _old_cells() == D.ALL_K5_CELLS and len(D.ALL_K5_CELLS) == 12


def test_coverage_premises_bite():
    """An altered copy of the restated rule -- four lanes up to a mean degree of 150 instead of 100 -- no longer covers the
    eight-lane column: the coverage assert depends on the rule, not on the table."""
    rule = lambda n_obs, n, m: D.k5_cell(n_obs, n, m, g_limits=(40.0, 150.0))
    altered = _cells(rule)
    assert altered != D.K5_CELL
    assert set(altered.values()) | _old_cells(rule) != D.ALL_K5_CELLS
    assert not any(G == 8 for G, _ in altered.values())


# ---------------------------------------------------------------- 3: conditioning
def test_slot_forms_are_honoured_on_tall_1500x80():
    """MVBA_SCHUR=slots / lanes are taken only while all lists of a range fit one XCD: 288 waves of 21 lists."""
    n, m, pt_ptr, cam, _ = _lists("tall_1500x80")
    _, S, slot_waves = V.size_pair_lists(V.pair_counts(pt_ptr, cam, m))
    assert slot_waves == 240 <= 32 * 9
    # ... and 96 waves of 64 lists (tests/test_gpu_schur_lanes.py::_lane_waves)
    assert -(-int(np.trace(S)) // 64) + -(-int(S[np.triu_indices(m, 1)].sum()) // 64) == 79 <= 96


@pytest.mark.parametrize("name", D.CASES)
def test_oracle_system_is_positive_definite(name):
    g = D.oracle_for(name)
    g.linearize()
    E0 = g.cost()
    E1 = g.try_step(C)
    if g.m <= 300:
        w = np.linalg.eigvalsh(g.A)
        assert w.min() > 0 and w.max() / w.min() < 1e7, (w.min(), w.max())
    else:  # (the eigenvalues of a matrix of order 5816 are not worth their time)
        np.linalg.cholesky(g.A)
    assert np.isfinite(E1) and E1 < E0


@pytest.mark.parametrize("loss,scale", D.ROBUST_LOSSES)
@pytest.mark.parametrize("name", D.ROBUST_CASES)
def test_robust_trial_cost_is_determined_to_a_hundredth_of_its_gpu_bound(name, loss, scale):
    """Reference against itself: the trial cost of tests/_robust_ref.py at damping ROBUST_C with the sums inside every point
    taken in reversed order, to 1e-11 relative -- 100 x below the 1e-9 of tests/test_gpu_robust.py::_check_step.  (At that
    helper's default damping 1e-3 the Huber twin of wide_80x647_20 gives 7.2e-10: tests/_degree_cases.py.)"""
    from _robust_ref import RobustOracleEngine

    n, m, pt_ptr, cam, xy, f0, axis, *state = D.problem(name, D.outlier_xy(name))
    E1 = []
    for cam_, xy_ in ((cam, xy), D.reversed_inside_points(pt_ptr, cam, xy)):
        g = RobustOracleEngine(n, m, pt_ptr, cam_, xy_, f0, axis, loss=loss, loss_scale=scale)
        g.set_params(*state)
        g.linearize()
        E1.append(g.try_step(D.ROBUST_C))
    diff = abs(E1[0] - E1[1]) / E1[0]
    print(f"{name} {loss}: trial cost {E1[0]:.6e}, reversed order {diff:.3e} relative (bound {D.ROBUST_SELF_DIFF_BOUND:g})")
    assert diff <= D.ROBUST_SELF_DIFF_BOUND and g.w.min() < 0.5


# ---------------------------------------------------------------- 4: the covariance premise
def test_covariance_references_agree_on_tall_1500x80():
    """Reference against reference: the Schur route of tests/_covariance_ref.py against the QR of the whole Jacobian, to 1e-10 of
    the largest entry -- 100 x below the 1e-8 at which the GPU is held to the Schur route."""
    import _covariance_ref as CR

    prob = D.problem("tall_1500x80")
    a, b = CR.schur_covariance(*prob), CR.dense_covariance(*prob)
    for k in ("points", "cameras", "cameras_full"):
        err = np.abs(a[k] - b[k]).max() / np.abs(b[k]).max()
        print(f"tall_1500x80 {k}: Schur route against dense QR {err:.3e} (recorded {D.COV_REF_DIFF[k]:.1e}, bound 1e-10)")
        assert D.COV_REF_DIFF[k] <= 1e-10 and err <= 1e-10


# ---------------------------------------------------------------- 7: the triangulation margin
def test_triangulation_host_versus_host_difference_on_tall_6000x300():
    """eigh of the moment matrix against the SVD of the stacked rows on this very case (degree-300 points beside degree 3): the
    figure the GPU margin is 100 x of, as tests/test_init_cpu.py measures it for the scenes of tests/_init_cases.py."""
    import _init_ref as ref

    K, R, t, pt_ptr, cam, xy = D.tri_args("tall_6000x300")
    a, b = ref.triangulate(K, R, t, pt_ptr, cam, xy, 0, linear="eigh"), ref.triangulate(K, R, t, pt_ptr, cam, xy, 0, linear="svd")
    assert (a[2] == 0).all() and (b[2] == 0).all()
    d = np.abs(a[0] - b[0]).max()
    print(f"tall_6000x300: eigh vs SVD max |dX| = {d:.3e} (recorded {D.TRI_HOST_DIFF:.1e})")
    assert 0.5 * D.TRI_HOST_DIFF <= d <= D.TRI_HOST_DIFF
    a2, b2 = D.tri_reference(), ref.triangulate(K, R, t, pt_ptr, cam, xy, 2, linear="svd")
    assert np.abs(a2[0] - b2[0]).max() <= D.TRI_HOST_DIFF
