"""NumPy restatement of mvba_match_descriptors: the int64 distance matrix, the lexicographic argmin, rules 1 to 4
and the counts.  Test infrastructure only."""
import numpy as np

COUNTS = ("n_matches", "n_queries", "n_no_candidate", "n_far", "n_ambiguous", "n_not_mutual")
KEPT, NO_CANDIDATE, FAR, AMBIGUOUS, NOT_MUTUAL = range(5)


def distance2(A, B):
    """(n_a, n_b) int64: the squared Euclidean distances of uint8 rows, exactly."""
    A, B = A.astype(np.int64), B.astype(np.int64)
    return (A * A).sum(axis=1)[:, None] + (B * B).sum(axis=1)[None, :] - 2 * (A @ B.T)


def nearest_two(D):
    """(best, best2, second2) (n_a,) int32 of a distance matrix: the column of the smallest (distance, column), its distance, and
    the smallest distance over the other columns; -1 where there is none."""
    na, nb = D.shape
    best, best2, second2 = np.full(na, -1, np.int32), np.full(na, -1, np.int32), np.full(na, -1, np.int32)
    if nb == 0 or na == 0:
        return best, best2, second2
    b = np.argmin(D, axis=1)  # (the first of equal minima: the smaller index)
    rows = np.arange(na)
    best[:], best2[:] = b, D[rows, b]
    if nb > 1:
        rest = D.copy()
        rest[rows, b] = np.iinfo(np.int64).max
        second2[:] = rest.min(axis=1)
    return best, best2, second2


def match_pair(A, B, ratio=None, mutual=True, max_dist2=-1):
    """One directed pair: queries A (n_a, dim), candidates B (n_b, dim).  Returns (kp_pairs (n, 2) int32, dist2 (n,) int32,
    best, best2, second2 (n_a,) int32, code (n_a,): 0 matched, else the first rule that rejected the query)."""
    D = distance2(A, B)
    best, best2, second2 = nearest_two(D)
    na, nb = D.shape
    code = np.zeros(na, np.int64)
    if nb == 0:
        code[:] = NO_CANDIDATE
    else:
        back = np.argmin(D, axis=0) if na else np.zeros(nb, np.int64)  # the best of every candidate among the queries, ties to the smaller index
        r2 = None if ratio is None else np.float64(ratio) * np.float64(ratio)
        for a in range(na):
            if max_dist2 >= 0 and best2[a] > max_dist2:
                code[a] = FAR
            elif r2 is not None and (second2[a] < 0 or not np.float64(best2[a]) < r2 * np.float64(second2[a])):
                code[a] = AMBIGUOUS
            elif mutual and back[best[a]] != a:
                code[a] = NOT_MUTUAL
    keep = np.nonzero(code == KEPT)[0]
    return np.stack([keep, best[keep]], axis=1).astype(np.int32), best2[keep].astype(np.int32), best, best2, second2, code


def match_descriptors(kp_ptr, desc, pairs, ratio=None, mutual=True, max_dist2=-1):
    """The whole call, in the form of lib._mvba.match_descriptors(want_nn=True) without the timings, plus ``code`` (Q,)."""
    kp_ptr, pairs = np.asarray(kp_ptr, np.int64), np.asarray(pairs, np.int64).reshape(-1, 2)
    parts = [match_pair(desc[kp_ptr[k]:kp_ptr[k + 1]], desc[kp_ptr[l]:kp_ptr[l + 1]], ratio, mutual, max_dist2) for k, l in pairs]
    cat = lambda i, shape, dtype: np.concatenate([p[i] for p in parts] + [np.zeros(shape, dtype)])
    code = cat(5, 0, np.int64)
    out = {"match_ptr": np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64),
           "kp_pairs": cat(0, (0, 2), np.int32), "dist2": cat(1, 0, np.int32), "nn_best": cat(2, 0, np.int32), "nn_dist2": cat(3, 0, np.int32),
           "nn_second2": cat(4, 0, np.int32), "code": code}
    out.update(n_matches=int((code == KEPT).sum()), n_queries=len(code), n_no_candidate=int((code == NO_CANDIDATE).sum()),
               n_far=int((code == FAR).sum()), n_ambiguous=int((code == AMBIGUOUS).sum()), n_not_mutual=int((code == NOT_MUTUAL).sum()))
    return out
