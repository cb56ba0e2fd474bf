"""mvba_two_view_robust at its structural limits ("Structural limits"): a scan with two chunks per thread over
chunk counts 0, 1, partial and 256; refit loops whose inlier set moves, is rejected after accepted changes, and that end at
different refits inside one tile; statuses 0, 1 and 2 next to each other; a count table that mixes degenerate and good
hypotheses; the maximum hypothesis count.  Integer outputs EXACTLY the NumPy restatement's (tests/test_ransac_cpu.py asserts
the premises, and each case's structural premise, on the reference alone), F and the Sampson RMS within 100 x the
host-versus-host difference of the very case (tests/_ransac_cases.py)."""
import numpy as np
import pytest

import _ransac_cases as RC
from lib import _mvba

pytestmark = pytest.mark.gpu

KEYS = ("F", "quality", "n_shared", "n_inliers", "best", "status", "inlier", "hyp_count")


def _run(pt_ptr, cam, xy, m, pairs, thr, H, seed, n_refit):
    return _mvba.two_view_robust(pt_ptr, cam, xy, m, pairs, thr, n_hypotheses=H, seed=seed, n_refit=n_refit, return_counts=True)


def _assert_exact(got, want, what):
    for key in ("hyp_count", "best", "n_shared", "n_inliers", "status", "inlier"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")


def _assert_close(got, want, margin, scale_xy, what):
    """F, Sampson RMS (relative to its own size; to the observations' where a minimal set is fitted exactly) and ratio of the
    pairs of status 0 within ``margin``; the other pairs NaN, without inliers."""
    ok = want["status"] == 0
    bad = ~ok
    assert np.isnan(got["F"][bad]).all() and np.isnan(got["quality"][bad]).all()
    assert not got["inlier"][bad].any() and not got["n_inliers"][bad].any() and (got["best"][bad] == -1).all()
    if not ok.any():
        return 0.0
    d = np.abs(got["F"][ok] - want["F"][ok]).max()
    scale = np.where(want["n_inliers"][ok] > 8, want["quality"][ok, 0], scale_xy)
    dq = (np.abs(got["quality"][ok, 0] - want["quality"][ok, 0]) / scale).max()
    dr = np.abs(got["quality"][ok, 1] - want["quality"][ok, 1]).max()
    print(f"{what}: max |dF| {d:.3e}, Sampson RMS relative {dq:.3e}, ratio {dr:.3e} (margin {margin:.1e})")
    assert d <= margin and dq <= margin and dr <= margin
    return d


def _assert_same_rows(a, rows_a, b, rows_b, what):
    """The pairs ``rows_a`` of call a are bitwise the pairs ``rows_b`` of call b, in every output."""
    for key in KEYS:
        x, y = np.ascontiguousarray(a[key][rows_a]), np.ascontiguousarray(b[key][rows_b])
        assert x.tobytes() == y.tobytes(), f"{what}: {key}"


@pytest.mark.parametrize("name", sorted(RC.LIMITS))
def test_limit_case(name):
    pt_ptr, cam, xy, m, pairs, thr, H, seed, n_refit = RC.limit_case(name)
    got, want = _run(pt_ptr, cam, xy, m, pairs, thr, H, seed, n_refit), RC.limit_reference(name)
    _assert_exact(got, want, name)
    _assert_close(got, want, RC.MARGIN * RC.RANSAC_HOST_DIFF[name], np.abs(xy).max(), name)
    st, hc = got["status"], got["hyp_count"]
    if name == "scan257":  # off[], the wave prefix and id[]: the inlier rows above; and the two orders of one pair
        assert got["n_shared"][1] == got["n_shared"][2] and got["n_shared"][1] % 256 != 0
        assert got["inlier"][1].sum() == got["inlier"][2].sum() == got["n_inliers"][1] and not np.array_equal(hc[1], hc[2])
        assert not got["inlier"][0][~RC.scan_keep()].any()  # no point outside the shared list
    elif name == "mixed":
        assert set(st.tolist()) == {0, 1, 2}
        alone = _run(pt_ptr, cam, xy, m, pairs[st == 0], thr, H, seed, n_refit)
        _assert_same_rows(got, st == 0, alone, slice(None), "the status-0 pairs among the others and alone")
    elif name == "mixed65":
        assert (got["n_shared"][st == 1] >= 1).all() and (hc[st == 1] == -1).all()
        alone = _run(pt_ptr, cam, xy, m, pairs[st == 0], thr, H, seed, n_refit)
        _assert_same_rows(got, st == 0, alone, slice(None), "the status-0 pairs among the others and alone")
    elif name == "partly_degenerate":  # the good path of k_ransac_hyp and the NaN rule of k_ransac_score in one 64-block
        assert (hc == -1).any() and (hc >= 8).any() and got["best"][0] == np.argmax(hc[0]) > 0 and hc[0, 0] == -1


@pytest.mark.parametrize("name", ["refits_1.5e-3", "refits_3e-3"])
def test_refit_counts_and_pairs_alone(name):
    """n_refit = 0, 1, 2, 3, 16 against the reference at the same n_refit; a pair of the three-pair call is bitwise the pair alone
    (its neighbours leave the loop at other refits: no state leaks inside a tile)."""
    pt_ptr, cam, xy, m, pairs, thr, H, seed, _ = RC.limit_case(name)
    for r in RC.REFIT_COUNTS:
        got, want = _run(pt_ptr, cam, xy, m, pairs, thr, H, seed, r), RC.limit_reference(name, "eigh", r)
        _assert_exact(got, want, f"{name}, n_refit = {r}")
        # the host-versus-host figure of this very n_refit (at 0 the hypothesis's own conditioning enters F), no less than the case's
        host = np.abs(want["F"] - RC.limit_reference(name, "svd", r)["F"]).max()
        _assert_close(got, want, RC.MARGIN * max(host, RC.RANSAC_HOST_DIFF[name]), np.abs(xy).max(), f"{name}, n_refit = {r}")
        if r == 0:
            np.testing.assert_array_equal(got["n_inliers"], want["hyp_count"].max(axis=1))
    for p in range(len(pairs)):
        one = _run(pt_ptr, cam, xy, m, pairs[p:p + 1], thr, H, seed, 16)
        _assert_same_rows(got, slice(p, p + 1), one, slice(None), f"{name}: pair {pairs[p].tolist()} in the call and alone")


def test_maximum_hypothesis_count():
    """n_hypotheses = 65 536 on "300x8" pair (0, 1): 1024 hypothesis blocks, gridDim.y of the scoring launch."""
    pt_ptr, cam, xy, m, pairs, thr, H, seed, _ = RC.case("300x8")
    got = _run(pt_ptr, cam, xy, m, pairs[:1], thr, RC.MAX_HYP, seed, 2)
    low = _run(pt_ptr, cam, xy, m, pairs[:1], thr, 512, seed, 2)
    hc = got["hyp_count"][0]
    assert hc.shape == (RC.MAX_HYP,) and got["status"][0] == 0 and got["n_shared"][0] == 80
    assert hc[:512].tobytes() == low["hyp_count"][0].tobytes()  # a hypothesis depends on (seed, k, l, h) only
    np.testing.assert_array_equal(hc[:512], RC.reference("300x8")["hyp_count"][0])
    hs, counts, _, _ = RC.max_hyp_reference()
    np.testing.assert_array_equal(hc[hs], counts)
    assert ((hc == -1) | (hc >= 8)).all() and got["best"][0] == np.argmax(hc)  # (argmax: the lowest h on ties)
    # the winner's own count, evaluated by the reference for that h alone
    _, xk, xl = RC.T.shared(pt_ptr, cam, np.asarray(xy).reshape(-1, 2), 0, 1)
    b = int(got["best"][0])
    assert RC.RR.hypothesis_counts(xk, xl, 0, 1, thr, seed, [b])[0][0] == hc[b] == hc.max()
    print(f"H = 65536: best {b} with count {hc.max()} of 80 shared points ({(hc == hc.max()).sum()} hypotheses reach it), {len(hs)} counts compared with the reference")
