"""Inputs shared by test_match_cpu.py and test_gpu_match.py, each built once: the descriptor sets of DESIGN.md §25 with the
settings they are matched under, their references, and the scene with descriptors for the end-to-end test.  Test
infrastructure only."""
import functools
from types import SimpleNamespace

import numpy as np

import _match_ref as MR
import _tracks_cases as TRC

TQ = 128     # csrc/mvba_match_host.h: MATCH_TQ, the queries of a workgroup
TC = 128     # MATCH_TC, the candidates of an LDS tile
KSTEP = 32   # MATCH_KSTEP, the bytes of a k step

N_K = (1, TQ - 1, TQ, TQ + 1, 2 * TQ + 3)
N_L = (1, 2, 31, 32, 33, TC - 1, TC, TC + 1, 2 * TC + 5)
DIMS = (16, 32, 48, 128, 496, 512)
FLAT_D2 = 512 * 255 ** 2  # 33 292 800: the largest distance there is


def _case(arrays, pairs, ratio=None, mutual=True, max_distance=None):
    """(kp_ptr, desc, pairs, kw): kw as tests/_match_ref.match_descriptors and lib._mvba.match_descriptors take it."""
    kp_ptr = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)
    desc = np.ascontiguousarray(np.concatenate(arrays), dtype=np.uint8)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    for a in (kp_ptr, desc, pairs):
        a.setflags(write=False)
    kw = {"ratio": ratio, "mutual": mutual, "max_dist2": -1 if max_distance is None else int(np.floor(max_distance ** 2))}
    return kp_ptr, desc, pairs, kw


def _tiles():
    """Images 0 .. 4 have N_K keypoints and images 5 .. 13 N_L: every (query, candidate) size on either side of a workgroup's
    queries and of an LDS tile, all 45 pairs in one call."""
    rng = np.random.default_rng(25)
    arrays = [rng.integers(0, 256, (n, 128), dtype=np.uint8) for n in N_K + N_L]
    return _case(arrays, [(i, len(N_K) + j) for i in range(len(N_K)) for j in range(len(N_L))], ratio=0.95)


def _dim(dim):
    rng = np.random.default_rng(dim)
    return _case([rng.integers(0, 256, (70, dim), dtype=np.uint8), rng.integers(0, 256, (45, dim), dtype=np.uint8)], [(0, 1), (1, 0)], ratio=0.95)


def _flat(changed, dim=512):
    """All bytes 0 against all bytes 255 (at dim 512 unless said); with ``changed`` one byte of candidate 17 is 254."""
    A, B = np.zeros((40, dim), np.uint8), np.full((37, dim), 255, np.uint8)
    if changed:
        B[17, 300 % dim] = 254
    return _case([A, B], [(0, 1), (1, 0)])


ORIENT_N = 50


def _orientation():
    """B[perm[a]] = A[a] with one byte raised by a + 1 (A stays below 200), among 10 unrelated rows: best(a) = perm[a] at distance
    (a + 1)^2, and the distance matrix is far from symmetric."""
    rng = np.random.default_rng(7)
    A = rng.integers(0, 200, (ORIENT_N, 128)).astype(np.uint8)
    perm = rng.permutation(ORIENT_N + 10)[:ORIENT_N]
    B = rng.integers(0, 256, (ORIENT_N + 10, 128)).astype(np.uint8)
    B[perm] = A
    B[perm, np.arange(ORIENT_N) % 128] += (np.arange(ORIENT_N) + 1).astype(np.uint8)
    return _case([A, B], [(0, 1)], mutual=False), perm


def _dup_candidates():
    """Every candidate comes twice (rows 2 i and 2 i + 1); query a is candidate pair a with a little noise."""
    rng = np.random.default_rng(8)
    base = rng.integers(8, 248, (30, 128))
    A = (base + rng.integers(-3, 4, base.shape)).astype(np.uint8)
    return _case([A, np.repeat(base, 2, axis=0).astype(np.uint8)], [(0, 1)], ratio=1.0)


def _dup_queries():
    """Queries 2 i and 2 i + 1 are the same row; candidate i is that row with a little noise."""
    rng = np.random.default_rng(9)
    base = rng.integers(8, 248, (30, 128))
    B = (base + rng.integers(-3, 4, base.shape)).astype(np.uint8)
    return _case([np.repeat(base, 2, axis=0).astype(np.uint8), B], [(0, 1)])


RULES_MAX_DISTANCE = 300.0


def _rules(**kw):
    """Image 0: 40 queries.  Image 1: candidates 0 .. 19 are queries 0 .. 19 shuffled, noise +-3 (matches); 20 .. 24 are queries
    20 .. 24 with noise +-60 (beyond max_distance); 25 and 26 are both query 25 with noise +-20 (ambiguous); 27 is query 26
    with noise +-10, and query 27 is query 26 with noise +-30 (27's best is 27, whose own best is 26: not mutual); 28, 29 random.
    Image 2 is empty, image 3 has one keypoint.  Pairs: forwards, from the empty image, to the empty image, to the single
    keypoint, both turned round."""
    rng = np.random.default_rng(10)
    A = rng.integers(64, 192, (40, 128))
    A[27] = A[26] + rng.integers(-30, 31, 128)
    B = rng.integers(0, 256, (30, 128))
    B[:20] = A[rng.permutation(20)] + rng.integers(-3, 4, (20, 128))
    B[20:25] = A[20:25] + rng.integers(-60, 61, (5, 128))
    B[25:27] = A[25] + rng.integers(-20, 21, (2, 128))
    B[27] = A[26] + rng.integers(-10, 11, 128)
    arrays = [np.clip(A, 0, 255).astype(np.uint8), np.clip(B, 0, 255).astype(np.uint8), np.zeros((0, 128), np.uint8),
              rng.integers(0, 256, (1, 128), dtype=np.uint8)]
    return _case(arrays, [(0, 1), (2, 1), (0, 2), (0, 3), (1, 0), (3, 0)], **kw)


WIDTH_N = 65600
WIDTH_BEST = (0, 65535, 65599)


def _index_width():
    """65 600 candidates of 16 bytes; the three queries are candidates 0, 65 535 and 65 599 themselves."""
    rng = np.random.default_rng(16)
    B = rng.integers(0, 256, (WIDTH_N, 16), dtype=np.uint8)
    return _case([B[list(WIDTH_BEST)].copy(), B], [(0, 1)])


CASES = {"tiles": _tiles, "flat": lambda: _flat(False), "flat_one": lambda: _flat(True), "orientation": lambda: _orientation()[0],
         "dup_candidates": _dup_candidates, "dup_queries": _dup_queries,
         "rules": lambda: _rules(ratio=0.8, max_distance=RULES_MAX_DISTANCE), "rules_no_ratio": lambda: _rules(max_distance=RULES_MAX_DISTANCE),
         "rules_one_way": lambda: _rules(ratio=0.8, mutual=False, max_distance=RULES_MAX_DISTANCE), "rules_any_distance": lambda: _rules(ratio=0.8), "rules_plain": _rules,
         "index_width": _index_width}
CASES.update({f"dim{d}": functools.partial(_dim, d) for d in DIMS})
LARGEST = ("tiles", "index_width")  # the most queries and pairs; the most keypoints
CHUNK_ROWS = 1 << 22  # csrc/mvba_match_host.h: MATCH_CHUNK_QUERIES, the query rows (both directions) of a chunk of pairs
CHUNK_PAIRS = 70      # copies of the index-width pair (65 603 rows each with the mutual check) that no longer fit one chunk


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    kp_ptr, desc, pairs, kw = case(name)
    return MR.match_descriptors(kp_ptr, desc, pairs, **kw)


@functools.lru_cache(maxsize=None)
def orientation_perm():
    return _orientation()[1]


# ---- the structural limits of the kernels ("Limits pass") ---------------------------------------------------
# Cases of their own, beside CASES: LARGEST keeps naming the largest members of CASES.
LIMIT_DIMS = tuple(range(16, 513, 16))  # every dim the entry point takes: every k-step count, full and partial
FLAT_DIMS = (16, 64, 256, 496, 512)     # the flat extremes: KS = 1, 2, 8, 16 (partial), 16


def ksteps(dim):
    """csrc/mvba_match.h: match_ksteps, the instantiation a dim runs -- the smallest power of two with 32 KS >= dim."""
    ks = 1
    while KSTEP * ks < dim:
        ks *= 2
    return ks


def lane_of_row(row):
    """(lane half, accumulator register) that holds candidate ``row`` of its image: the C/D map of DESIGN.md §25 inside the row's 32
    of an MFMA tile, row = (reg & 3) + 8 (reg >> 2) + 4 half."""
    r = row % 32
    half, reg = (r >> 2) & 1, (r & 3) + 4 * (r >> 3)
    assert r == (reg & 3) + 8 * (reg >> 2) + 4 * half
    return half, reg


TIE_NC = 300   # candidates of an image: LDS tiles of 128, 128 and 44
TIE_NQ = 33    # queries of an image: waves 0 and 1 of the workgroup
TIE_POS = (0, 1, 3, 4, 7, 8, 12, 15, 16, 28, 31, 32, 36, 63, 64, 127, 128, 132, 255, 256, 260, 299)
# (byte 0 of row i raised by, byte 1 of row j lowered by), i < j: the two rows differ, and so do their norms
TIE_VARIANTS = {"tie": (3, 3), "near_first": (3, 4), "near_last": (4, 3)}
TIE_TRIPLES = ((4, 132, 260), (31, 128, 256), (127, 255, 299), (12, 200, 257))  # one row in each LDS tile
TIE_TRIPLE_VARIANTS = {"tie3": (3, 3, 3), "mid3": (4, 3, 4)}  # byte 0 raised, byte 1 lowered, byte 2 raised
TIE_FAR = 16   # every row that is not planted is farther than this from the query


def tie_rounds():
    """The 231 pairs i < j of TIE_POS as 21 rounds of 11 disjoint pairs (the circle method): a round is one candidate image."""
    n = len(TIE_POS)
    rounds = []
    for r in range(n - 1):
        ring = [n - 1] + [(r + k) % (n - 1) for k in range(n - 1)]
        rounds.append([tuple(sorted((TIE_POS[ring[k]], TIE_POS[ring[n - 1 - k]]))) for k in range(n // 2)])
    return rounds


@functools.lru_cache(maxsize=None)
def ties():
    """(case, expect).  dim 16, no ratio, one way.  Query images 0 .. 20 (one per round of tie_rounds) and 21 (the triples), TIE_NQ
    random rows each; then the candidate images, TIE_NC random rows each: per round one for every variant of TIE_VARIANTS, and one
    for every variant of TIE_TRIPLE_VARIANTS.  In the image of (round, variant) the pair k = (i, j) of the round belongs to ONE query
    row Z (the rows of a query image are dealt out by a permutation, so that planted queries fall into both waves): row i is Z
    with byte 0 raised, row j is Z with byte 1 lowered, by the variant's amounts.  The other 22 query rows of that pair of images
    meet random rows only.  expect: a list of (variant, planted rows, the query's row in the call's Q, best, best2, second2)."""
    rng = np.random.default_rng(2)
    rounds = tie_rounds()
    n_q = len(rounds) + 1
    queries = [rng.integers(8, 248, (TIE_NQ, 16)).astype(np.uint8) for _ in range(n_q)]
    cands, pairs, expect = [], [], []

    def image(name, q, slots, rows_of, amounts, bytes_sign):
        B = rng.integers(0, 256, (TIE_NC, 16)).astype(np.uint8)
        for k, rows in enumerate(rows_of):
            a = int(slots[k])
            Z = queries[q][a].astype(np.int64)
            for row, amount, (byte, sign) in zip(rows, amounts, bytes_sign):
                B[row] = Z
                B[row, byte] = Z[byte] + sign * amount
            d2 = sorted(amount * amount for amount in amounts)
            best = rows[int(np.argmin(amounts))]  # (argmin: the first of equal amounts, the smaller row)
            expect.append((name, tuple(rows), len(pairs) * TIE_NQ + a, best, d2[0], d2[1]))
        pairs.append((q, n_q + len(cands)))
        cands.append(B)

    for q, rnd in enumerate(rounds):
        slots = rng.permutation(TIE_NQ)
        for v, (name, amounts) in enumerate(TIE_VARIANTS.items()):
            image(name, q, slots[11 * v:11 * v + 11], rnd, amounts, ((0, 1), (1, -1)))
    slots = rng.permutation(TIE_NQ)
    for v, (name, amounts) in enumerate(TIE_TRIPLE_VARIANTS.items()):
        image(name, n_q - 1, slots[4 * v:4 * v + 4], TIE_TRIPLES, amounts, ((0, 1), (1, -1), (2, 1)))
    return _case(queries + cands, pairs, mutual=False), expect


WAVE_NQ = (31, 32, 33, 63, 64, 65, 95, 96, 97)  # either side of every wave's 32 queries of a workgroup
WAVE_NC = (1, 33, 129)


def _waves():
    """Images 0 .. 8 have WAVE_NQ keypoints, images 9 .. 11 WAVE_NC: all 27 pairs in one call, dim 128."""
    rng = np.random.default_rng(33)
    arrays = [rng.integers(0, 256, (n, 128), dtype=np.uint8) for n in WAVE_NQ + WAVE_NC]
    return _case(arrays, [(i, len(WAVE_NQ) + j) for i in range(len(WAVE_NQ)) for j in range(len(WAVE_NC))], ratio=0.95)


SCAN_BLOCK = 1024      # csrc/mvba_tracks.h: TRK_SCAN_BLOCK, the rows of a block of the scan
SCAN_SUMS = 256        # block totals k_tracks_scan_sums takes per trip
SCAN_NQ = (100_000, 0, 163_168, 1)  # 263 169 = 256 * 1024 + 1024 + 1 query rows: 258 blocks, the last holds the last image's one query
SCAN_NC = 5


@functools.lru_cache(maxsize=None)
def _scan_arrays():
    rng = np.random.default_rng(258)
    arrays = [rng.integers(0, 256, (n, 16), dtype=np.uint8) for n in SCAN_NQ + (SCAN_NC,)]
    arrays[4][2, 5] = 100
    arrays[3][0] = arrays[4][2]  # the one query of block 257: candidate 2 with one byte raised by 1 -- kept under every rule
    arrays[3][0, 5] = 101
    return arrays


def _scan(mutual):
    """Query images 0 .. 3 of SCAN_NQ rows (image 1 is empty), each against image 4's SCAN_NC candidates, ratio 0.9, dim 16."""
    return _case(_scan_arrays(), [(i, 4) for i in range(4)], ratio=0.9, mutual=mutual)


LIMIT_CASES = {f"k{d:03d}": functools.partial(_dim, d) for d in LIMIT_DIMS}
LIMIT_CASES.update({f"flat{d:03d}": functools.partial(_flat, False, d) for d in FLAT_DIMS})
LIMIT_CASES.update({f"flat_one{d:03d}": functools.partial(_flat, True, d) for d in FLAT_DIMS})
LIMIT_CASES.update({"ties": lambda: ties()[0], "waves": _waves, "scan258": lambda: _scan(False), "scan258_mutual": lambda: _scan(True)})


@functools.lru_cache(maxsize=None)
def limit_case(name):
    return LIMIT_CASES[name]()


@functools.lru_cache(maxsize=None)
def limit_reference(name):
    kp_ptr, desc, pairs, kw = limit_case(name)
    return MR.match_descriptors(kp_ptr, desc, pairs, **kw)


# ---- end to end: a scene with descriptors ---------------------------------------------------------------------------------
E2E_RATIO = 0.8
E2E_SEED = 25
E2E_TWINS = 20   # points that share their descriptor with another point: repeated structure
E2E_NOISE = 8    # uniform integer noise of an observation's descriptor about its point's


@functools.lru_cache(maxsize=None)
def scene_descriptors():
    """The scene of _tracks_cases with its keypoints shuffled and 5 unmatched ones per image (matcher_output, no wrong matches), and a
    128-byte descriptor per keypoint: its point's base plus noise, random bytes for an unmatched one.  Returns a namespace:
    ``mo`` (the matcher output: keypoints, the TRUE matches), ``descriptors`` (a list of (n_i, 128) uint8), ``point_of_kp`` (a list of
    (n_i,): the scene point, -1 unmatched), ``twin`` (n_points,): the point whose base a point carries (itself unless a twin)."""
    sc, mo = TRC.scene(), TRC.scene_matches(0.0)
    rng = np.random.default_rng(E2E_SEED)
    base = rng.integers(0, 256, (sc.n_points, 128))
    pick = rng.permutation(sc.n_points)[:2 * E2E_TWINS]
    twin = np.arange(sc.n_points)
    twin[pick[:E2E_TWINS]] = pick[E2E_TWINS:]
    base = base[twin]
    pt = np.repeat(np.arange(sc.n_points), np.diff(sc.pt_ptr))
    descriptors, point_of_kp = [], []
    for i in range(8):
        n = len(mo.keypoints[i])
        obs = np.nonzero(sc.cam_idx == i)[0]
        point = np.full(n, -1, np.int64)
        point[mo.kp_of_obs[obs]] = pt[obs]
        d = rng.integers(0, 256, (n, 128))
        seen = point >= 0
        d[seen] = np.clip(base[point[seen]] + rng.integers(-E2E_NOISE, E2E_NOISE + 1, (int(seen.sum()), 128)), 0, 255)
        descriptors.append(d.astype(np.uint8))
        point_of_kp.append(point)
    return SimpleNamespace(mo=mo, descriptors=descriptors, point_of_kp=point_of_kp, twin=twin)


def scene_pairs():
    return [(k, l) for k in range(8) for l in range(k + 1, 8)]


@functools.lru_cache(maxsize=None)
def scene_reference(ratio):
    """{(k, l): (n, 2) int64} of the reference on the scene's descriptors, every k < l, mutual."""
    sd = scene_descriptors()
    kp_ptr = np.concatenate([[0], np.cumsum([len(d) for d in sd.descriptors])])
    ref = MR.match_descriptors(kp_ptr, np.concatenate(sd.descriptors), scene_pairs(), ratio=ratio, mutual=True)
    return {kl: ref["kp_pairs"][ref["match_ptr"][i]:ref["match_ptr"][i + 1]].astype(np.int64) for i, kl in enumerate(scene_pairs())}


def scene_score(matches):
    """(true matches found, matches between twins, other wrong matches, true matches there are) of a dict of matches."""
    sd = scene_descriptors()
    true = same = other = 0
    for (k, l), idx in matches.items():
        p, q = sd.point_of_kp[k][idx[:, 0]], sd.point_of_kp[l][idx[:, 1]]
        t = (p >= 0) & (p == q)
        s = ~t & (p >= 0) & (q >= 0) & (sd.twin[np.maximum(p, 0)] == sd.twin[np.maximum(q, 0)])
        true, same, other = true + int(t.sum()), same + int(s.sum()), other + int((~t & ~s).sum())
    return true, same, other, sd.mo.n_true
