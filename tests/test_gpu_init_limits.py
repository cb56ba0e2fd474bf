"""mvba_triangulate, mvba_project and mvba_resect at the sizes where their launch arithmetic changes ("Structural
limits"): the second trip of k_triangulate's grid-stride loop, the LDS camera table above 64 KiB and at its cap, resection
with more than 256 cameras, full and one-element chunks, cameras without a chunk, nothing usable at all, and inputs that
make a Hartley scale infinite.  Parity margins are those of tests/test_gpu_init.py (100 x the scene's host-versus-host
difference; the new scenes are entries of TRI_HOST_DIFF / RESECT_HOST_DIFF and run through test_triangulate_parity and
test_resect_parity there); everything else here is bitwise or integer-exact: the kernels use no floating-point atomics
and fixed summation orders."""
import numpy as np
import pytest

import _init_cases as C
import _init_ref as ref
from lib import _mvba

pytestmark = pytest.mark.gpu


def _bits(a):
    """The array as unsigned integers of its item size: equality is bitwise, NaN included."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def _assert_tiles_repeat(a, reps, what):
    a = _bits(a).reshape(reps, -1)
    bad = np.nonzero((a != a[0]).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {reps} tiles differ from tile 0, first tile {bad[0]}"


@pytest.mark.parametrize("n_refine, with_quality", [(2, True), (0, False)])
def test_triangulate_second_trip_of_the_grid_stride_loop(n_refine, with_quality):
    """More points than the grid has threads: every tile of the repeated 300 x 8 list must be bitwise tile 0 (a point's
    arithmetic does not depend on its index; tile 0 is held to the reference by test_triangulate_parity)."""
    reps, pt_ptr, cam, xy = C.tiled_scene()
    n = len(pt_ptr) - 1
    assert n > C.GRID_CAP and n - C.GRID_CAP >= 300  # the premise: a second trip that holds whole tiles
    K, R, t = C.tri_args("300x8")[:3]
    if with_quality:
        X, q, st, _ = _mvba.triangulate(K, R, t, pt_ptr, cam, xy, n_refine=n_refine)
        _assert_tiles_repeat(q, reps, "quality")
        _assert_tiles_repeat(st, reps, "status")
        assert (st[:300] == 0).all()
    else:  # quality = NULL, status = NULL: the kernel's other two branches
        import ctypes

        lib = _mvba.load_library()
        X = np.full((n, 3), -7.0)
        rc = lib.mvba_triangulate(_mvba._ptr(K), _mvba._ptr(R), _mvba._ptr(t), 8, n, pt_ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  cam.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _mvba._ptr(xy), len(cam), n_refine, _mvba._ptr(X),
                                  None, None, None, -1)
        _mvba.raise_for(rc, lib)
    _assert_tiles_repeat(X, reps, "X")
    X0 = _mvba.triangulate(*C.tri_args("300x8"), n_refine=n_refine)[0]
    assert _bits(X[:300]).tobytes() == _bits(X0).tobytes()  # tile 0 is the 300-point call


def test_project_of_triangulate_at_the_camera_cap():
    """m = 1704, noise-free: k_triangulate and k_project_obs both hold the 163 584-byte table; the round trip returns the
    observations (the form of test_project_of_triangulate_returns_the_observations)."""
    sc = C.tri_scene("300x1704")
    assert 12 * 8 * sc.n_images == 163584 and 12 * 8 * sc.n_images > 65536
    assert (sc.cam_idx == 1703).any() and (sc.cam_idx == 682).any() and (sc.cam_idx == 683).any()  # the last row, the rows at 64 KiB
    xy = C.exact_xy(sc)
    X, _, st, _ = _mvba.triangulate(sc.K_gt, sc.R_gt, sc.t_gt, sc.pt_ptr, sc.cam_idx, xy, n_refine=2)
    assert (st == 0).all()
    back = _mvba.project(X, sc.K_gt, sc.R_gt, sc.t_gt, sc.pt_ptr, sc.cam_idx)
    np.testing.assert_allclose(back, xy, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(X, sc.X_gt, rtol=0, atol=1e-12)


def test_camera_table_scenes_reach_the_rows_they_are_for():
    sc = C.tri_scene("300x683")
    assert 12 * 8 * 683 > 65536 >= 12 * 8 * 682 and (sc.cam_idx == 682).any()


def test_resect_cameras_without_observations_between_others():
    """m = 11 with cameras 1, 4, 10 unobserved (cam_ch_ptr[k] == cam_ch_ptr[k + 1]): status 1 and NaN for them, and the other
    eight bitwise the 8-camera call's."""
    X, pt_ptr, cam, xy, m, kept = C.empty_camera_case()
    P, q, st, _ = _mvba.resect(X, pt_ptr, cam, xy, m)
    P8, q8, st8, _ = _mvba.resect(*C.resect_case("300x8")[:5])
    empty = list(C.EMPTY_CAMERAS)
    assert (st[empty] == 1).all() and np.isnan(P[empty]).all() and np.isnan(q[empty]).all()
    assert (st8 == 0).all()
    np.testing.assert_array_equal(st[kept], st8)
    assert _bits(P[kept]).tobytes() == _bits(P8).tobytes() and _bits(q[kept]).tobytes() == _bits(q8).tobytes()


@pytest.mark.parametrize("how", ["point_ok", "nan"])
def test_resect_with_nothing_usable(how):
    """No usable observation (n_ch == 0): every camera status 1, all NaN, MVBA_OK, no device work."""
    X, pt_ptr, cam, xy, m, _ = C.resect_case("300x8")
    if how == "point_ok":
        P, q, st, tm = _mvba.resect(X, pt_ptr, cam, xy, m, point_ok=np.zeros(len(X), bool))
    else:
        P, q, st, tm = _mvba.resect(np.full_like(X, np.nan), pt_ptr, cam, xy, m)
    assert (st == 1).all() and np.isnan(P).all() and np.isnan(q).all() and tm["kernel"] == 0.0


@pytest.mark.parametrize("kind", sorted(C.COINCIDENT_POINTS))
def test_resect_coincident_image_points(kind):
    """Every observation of camera 3 at one image point: status 2, P NaN, the RMS NaN; with an exactly representable point
    the Hartley scale is infinite, the sums are NaN and there is no eigenvalue ratio either.  The other cameras are bitwise
    what they are on the untouched list."""
    X, pt_ptr, cam, xy0, m, _ = C.resect_case("300x8")
    xy, k = C.coincident_xy(kind), C.COINCIDENT_CAMERA
    assert (cam == k).sum() >= 6
    P, q, st, _ = _mvba.resect(X, pt_ptr, cam, xy, m)
    Pr, qr, sr = ref.resect(X, pt_ptr, cam, xy, m)
    np.testing.assert_array_equal(st, sr)
    assert st[k] == 2 and sr[k] == 2 and np.isnan(P[k]).all() and np.isnan(q[k, 0])
    if kind == "exact":
        assert np.isnan(q[k, 1]) and np.isnan(qr[k, 1])
    P0, q0, st0, _ = _mvba.resect(X, pt_ptr, cam, xy0, m)
    rest = np.arange(m) != k
    assert (st[rest] == 0).all() and _bits(P[rest]).tobytes() == _bits(P0[rest]).tobytes()
    assert _bits(q[rest]).tobytes() == _bits(q0[rest]).tobytes()


def test_triangulate_duplicated_observation():
    """A point whose two observations are the same camera twice: status 2 (no parallax), NaN; the run [2, 2] does not
    ascend, which the stateless call does not require.  Its neighbours are bitwise those of the list without it."""
    K, R, t, pt_ptr, cam, xy, expect = C.duplicate_observation_case()
    K0, R0, t0, pt_ptr0, cam0, xy0 = C.status_case()[:6]
    for n_refine in (0, 2):
        X, q, st, _ = _mvba.triangulate(K, R, t, pt_ptr, cam, xy, n_refine=n_refine)
        np.testing.assert_array_equal(st, expect)
        np.testing.assert_array_equal(ref.triangulate(K, R, t, pt_ptr, cam, xy, n_refine)[2], expect)
        assert st[5] == 2 and np.isnan(X[5]).all() and np.isnan(q[5]).all()
        X0, q0, st0, _ = _mvba.triangulate(K0, R0, t0, pt_ptr0, cam0, xy0, n_refine=n_refine)
        rest = np.arange(40) != 5
        assert _bits(X[rest]).tobytes() == _bits(X0[rest]).tobytes() and _bits(q[rest]).tobytes() == _bits(q0[rest]).tobytes()
