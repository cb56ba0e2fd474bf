"""mvba_covisibility and mvba_two_view at the sizes where their launch arithmetic changes ("Structural
limits"): the second trip of k_covisibility's grid-stride loop, its last LDS size (m = 128) next to the first
device-memory one (129), a combine lane that adds more than one chunk, more than one tile of pairs under either bound
(128 MiB of partials, gridDim.y), and pairs whose Hartley scale is 0 / 0 or infinite.  The parity of the 66-chunk scene
"16641x3" is an entry of TWOVIEW_HOST_DIFF and runs through test_fundamental_parity; everything here is bitwise or
integer-exact: the kernels use no floating-point atomics and fixed summation orders."""
import time

import numpy as np
import pytest

import _init_cases as IC
import _twoview_cases as C
import _twoview_ref as T
from lib import _mvba

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def _same(a, b):
    return _bits(a).tobytes() == _bits(b).tobytes()


def _assert_periodic(out, period, what):
    """Every occurrence of a pair is bitwise its first: out[i] == out[i % period] for F, quality, n_shared, status."""
    for name, a in zip(("F", "quality", "n_shared", "status"), out[:4]):
        a = _bits(a).reshape(len(a), -1)
        first = a[np.arange(len(a)) % period]
        bad = np.nonzero((a != first).any(axis=1))[0]
        assert bad.size == 0, f"{what} {name}: {bad.size} of {len(a)} entries differ from their first occurrence, first at {bad[0]}"


def test_covisibility_second_trip_of_the_grid_stride_loop():
    reps, pt_ptr, cam, _ = IC.tiled_scene()
    n = len(pt_ptr) - 1
    assert n > IC.GRID_CAP and n - IC.GRID_CAP >= 300  # the premise: more points than the grid has threads
    sc = C.scene("300x8")
    base, _ = _mvba.covisibility(sc.pt_ptr, sc.cam_idx, 8)
    np.testing.assert_array_equal(base, T.covisibility(sc.pt_ptr, sc.cam_idx, 8))
    count, _ = _mvba.covisibility(pt_ptr, cam, 8)
    assert count.dtype == np.int64
    np.testing.assert_array_equal(count, reps * base)


def test_covisibility_last_lds_size_and_first_beyond():
    """m = 128: the table is exactly 64 KiB, the last size in LDS; the same visibility plus one camera, m = 129, counts in
    device memory.  Both against the integer product, and equal on the common block."""
    assert 128 * 128 * 4 == 65536
    rng = np.random.default_rng(7)
    vis = rng.random((700, 129)) < 0.1  # 700 points: more than one workgroup flushes its table
    vis[:, [0, 127]] = True
    counts = {}
    for m in (128, 129):
        v = vis[:, :m]
        cam = np.nonzero(v)[1].astype(np.int32)
        pt_ptr = np.concatenate([[0], np.cumsum(v.sum(axis=1))]).astype(np.int64)
        counts[m], _ = _mvba.covisibility(pt_ptr, cam, m)
        np.testing.assert_array_equal(counts[m], v.T.astype(np.int64) @ v.astype(np.int64))
    np.testing.assert_array_equal(counts[129][:128, :128], counts[128])
    assert counts[128][127, 127] == 700 and counts[128][0, 127] == 700  # the last cell of the table


def test_more_than_64_chunks_list_and_dense_grid_agree():
    pt_ptr, cam, xy, m, pairs = C.case("16641x3")
    n = len(pt_ptr) - 1
    assert -(-n // C.TV_CHUNK) == 66 > 64 and n % C.TV_CHUNK == 1 and len(pairs) == 6
    a = _mvba.two_view(pt_ptr, cam, xy, m, pairs)
    b = _mvba.two_view(None, None, xy.reshape(n, m, 2), m, pairs)
    assert (a[3] == 0).all() and (a[2] == n).all()
    for u, v in zip(a[:4], b[:4]):
        assert _same(u, v)


def test_pair_tiles_under_the_partials_bound():
    """5700 pairs on 66 chunks: 128 MiB / (8 x 45 x 66) = 5648 pairs per launch, so the call takes two tiles (p0 > 0)."""
    pt_ptr, cam, xy, m, six = C.case("16641x3")
    n_pairs = 5700
    tile = C.pair_tile(len(pt_ptr) - 1, n_pairs)
    assert tile == (128 << 20) // (8 * 45 * 66) == 5648 and tile < C.TV_MAX_TILE and n_pairs > tile
    out = _mvba.two_view(pt_ptr, cam, xy, m, C.cycled(six, n_pairs))
    _assert_periodic(out, 6, "5700 pairs")
    assert (out[3] == 0).all()
    one = _mvba.two_view(pt_ptr, cam, xy, m, six)
    for u, v in zip(out[:4], one[:4]):
        assert _same(u[:6], v)


def test_pair_tiles_under_the_grid_bound():
    """65 600 pairs on 2 chunks: gridDim.y caps a launch at 65 535 pairs, the second tile holds 65."""
    pt_ptr, cam, xy, m, pairs = C.case("300x8")
    n_pairs = 65600
    tile = C.pair_tile(len(pt_ptr) - 1, n_pairs)
    assert tile == 65535 < (128 << 20) // (8 * 45 * 2) and n_pairs > tile
    t0 = time.perf_counter()
    out = _mvba.two_view(pt_ptr, cam, xy, m, C.cycled(pairs, n_pairs))
    dt = time.perf_counter() - t0
    print(f"65 600 pairs: {dt:.2f} s for the call, of which upload {out[4]['upload']:.0f} ms, kernels {out[4]['kernel']:.0f} ms, "
          f"rest (65 600 eigen-solves of order 9 on the host) {out[4]['download']:.0f} ms")
    _assert_periodic(out, len(pairs), "65 600 pairs")
    one = _mvba.two_view(pt_ptr, cam, xy, m, pairs)
    for u, v in zip(out[:4], one[:4]):
        assert _same(u[:len(pairs)], v)


def test_pair_without_shared_points():
    """Count 0 (the centroid is 0 / 0): n_shared 0, status 1, NaN; the other pairs of the call are bitwise what they are
    without it."""
    pt_ptr, cam, xy, m = C.no_shared_case()
    pairs = C.case("300x8")[4]
    with_it = np.concatenate([pairs[:7], np.array([(0, 8)], np.int32), pairs[7:], np.array([(8, 3)], np.int32)])
    a = _mvba.two_view(pt_ptr, cam, xy, m, with_it)
    b = _mvba.two_view(pt_ptr, cam, xy, m, pairs)
    empty = np.array([7, len(with_it) - 1])
    rest = np.setdiff1d(np.arange(len(with_it)), empty)
    F, q, ns, st = a[:4]
    assert (ns[empty] == 0).all() and (st[empty] == 1).all() and np.isnan(F[empty]).all() and np.isnan(q[empty]).all()
    assert (b[3] == 0).all()
    for u, v in zip(a[:4], b[:4]):
        assert _same(u[rest], v)
    np.testing.assert_array_equal(T.two_view(pt_ptr, cam, xy, m, [(0, 8)])[3], [1])


@pytest.mark.parametrize("kind", sorted(IC.COINCIDENT_POINTS))
def test_coincident_image_points(kind):
    """Every observation of camera 3 at one image point (zero spread: an infinite Hartley scale, then inf x 0): the pairs
    with camera 3 as k and as l come back status 2 with F and quality NaN and the right n_shared; the others are bitwise
    what they are on the untouched list."""
    pt_ptr, cam, xy0, m, pairs = C.case("300x8")
    pairs = np.concatenate([pairs, np.array([(6, 3)], np.int32)])
    xy, k = IC.coincident_xy(kind), IC.COINCIDENT_CAMERA
    hit = (pairs == k).any(axis=1)
    assert (pairs[hit][:, 0] == k).any() and (pairs[hit][:, 1] == k).any()  # the coincidence in k and in l
    F, q, ns, st, _ = _mvba.two_view(pt_ptr, cam, xy, m, pairs)
    Fr, qr, nr, sr = T.two_view(pt_ptr, cam, xy, m, pairs)
    np.testing.assert_array_equal(ns, nr)
    np.testing.assert_array_equal(st, sr)
    assert (ns[hit] >= 8).all() and (st[hit] == 2).all() and np.isnan(F[hit]).all() and np.isnan(q[hit]).all()
    b = _mvba.two_view(pt_ptr, cam, xy0, m, pairs)
    assert (st[~hit] == 0).all()
    for u, v in zip((F, q, ns, st), b[:4]):
        assert _same(u[~hit], v[~hit])
