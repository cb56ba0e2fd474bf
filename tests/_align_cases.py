"""Cases shared by test_align_cpu.py and test_gpu_align.py, each built once, and the host-versus-host differences (Horn's 4 x 4
eigen-problem by eigh against Umeyama's 3 x 3 SVD) that set the parity margins -- the rule of tests/_homography_cases.py.  Test
infrastructure only.

The construction is the issue's: src = make_scene(n, 3, vis_p=1.0).X_gt, dst = a fixed similarity of src (s = 2.5, a rotation from
a seeded QR, tau = (10, -3, 4)) plus Gaussian noise 1e-3 s, a seeded 30 % of the rows replaced by uniform positions in dst's
bounding box, threshold 0.01 s."""
import functools

import numpy as np

import _align_ref as AR
import _ransac_cases as RC
import _twoview_cases as C
from lib.synthetic import make_scene

MARGIN = C.MARGIN
# The smallest guard (_align_ref.inlier_test: |d^2 / thr^2 - 1|) a case may have for its integer outputs to be compared exactly.  A
# comparison d^2 <= thr^2 differs between the device (fused multiply-adds) and NumPy by the rounding of s Q x + tau - y relative to
# thr: a few eps |y| / thr = 4e-16 x 15 / 0.025 = 2e-13, squared-distance relative 5e-13 -- and by the model itself, which the two
# routes of the reference compute differently too: they must agree on every integer.  1e-7 is the bound the other RANSAC tests hold.
GUARD = 1e-7
SCALE, TAU, NOISE, THRESHOLD, FRACTION = 2.5, np.array([10.0, -3.0, 4.0]), 1e-3, 0.01, 0.3

# name: (n, s, n_hypotheses, seed, ok mask and NaN rows)
PARITY = {"a80": (80, SCALE, 512, 1, False), "a257": (257, SCALE, 512, 1, False), "a300": (300, SCALE, 512, 1, False),
          "rigid80": (80, 1.0, 512, 1, False), "masked300": (300, SCALE, 512, 2, True)}
# The clean rows each case's reference must return, and the replaced rows that land within the threshold of the clean fit by
# chance (none on these cases: a uniform position in a box of 2 x 2 x 2 s^3 hits a ball of radius 0.01 s with probability 5e-7).
N_CLEAN = {"a80": 56, "a257": 180, "a300": 210, "rigid80": 56, "masked300": 187}
# Host-versus-host max-abs difference of the final (s, Q, tau), measured by test_align_cpu.py on the very cases below; the plain fit
# of a case's clean rows differs by the same figure (it is the same fit).  A GPU parity assert gets MARGIN x its case's figure, the
# eigenvalue gap and the spread the same margin relative to their own size, the RMS residual rms_margin().
HOST_DIFF = {"a80": 1.2e-15, "a257": 2.8e-15, "a300": 2.3e-15, "rigid80": 4.5e-16, "masked300": 5.6e-16,
             # the structural limits
             "h64": 1.2e-15, "h65": 1.2e-15, "three": 1.8e-15, "scan256": 7.8e-16, "scan257": 3.9e-16, "scan513": 8.9e-16, "refits": 6.7e-16}
# A residual s Q x + tau - y is a difference of numbers of the size of y: a model that moves by d in every entry moves each
# component of it by at most d (1 + (1 + s) |x|_1), and the RMS by no more.  |x|_1 <= 3 on these scenes (|x_i| <= 1), s <= 2.5.
RESIDUAL_GAIN = 1.0 + (1.0 + 2.5) * 3.0


def rms_margin(name):
    """The absolute margin of the RMS residual: the model's margin carried through the residual."""
    return MARGIN * HOST_DIFF[name] * RESIDUAL_GAIN


def rotation(seed=4):
    Q = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))[0]
    return Q if np.linalg.det(Q) > 0 else -Q


def truth(s):
    return np.concatenate([[s], rotation().ravel(), TAU])


@functools.lru_cache(maxsize=None)
def correspondences(n, s, noise_seed=3, bad_seed=7):
    """(src, dst, bad): ``bad`` marks the replaced rows."""
    src = make_scene(n, 3, vis_p=1.0, project="numpy").X_gt.copy()
    rng = np.random.default_rng(noise_seed)
    dst = AR.transform(truth(s), src)[0] + rng.normal(0.0, NOISE * s, (n, 3))
    brng = np.random.default_rng(bad_seed)
    bad = np.zeros(n, bool)
    bad[brng.choice(n, int(round(FRACTION * n)), replace=False)] = True
    lo, hi = dst.min(axis=0), dst.max(axis=0)
    dst[bad] = lo + (hi - lo) * brng.random((int(bad.sum()), 3))
    for a in (src, dst, bad):
        a.setflags(write=False)
    return src, dst, bad


@functools.lru_cache(maxsize=None)
def case(name):
    """(src, dst, ok or None, with_scale, threshold, n_hypotheses, seed, clean): ``clean`` marks the usable rows that were not
    replaced.  "masked300": a seeded tenth of the rows forbidden by ok, rows 5 and 17 NaN in src and dst behind an ok that allows
    them, row 29 NaN and forbidden."""
    n, s, H, seed, masked = PARITY[name]
    src, dst, bad = correspondences(n, s)
    ok = None
    if masked:
        src, dst = src.copy(), dst.copy()
        ok = np.random.default_rng(11).random(n) >= 0.1
        ok[[5, 17]] = True
        ok[29] = False
        src[5, 1] = np.nan
        dst[17, 2] = np.inf
        src[29] = np.nan
        for a in (src, dst, ok):
            a.setflags(write=False)
    clean = AR.usable(src, dst, ok) & ~bad
    return src, dst, ok, s != 1.0, THRESHOLD * s, H, seed, clean


@functools.lru_cache(maxsize=None)
def reference(name, route="horn", n_refit=2, n_hyp=None):
    src, dst, ok, ws, thr, H, seed, _ = case(name)
    return AR.align_robust(src, dst, thr, ok, ws, H if n_hyp is None else n_hyp, seed, n_refit, route)


@functools.lru_cache(maxsize=None)
def plain_reference(name, route="horn"):
    """_align_ref.align on the clean rows of a case."""
    src, dst, _, ws, _, _, _, clean = case(name)
    return AR.align(src[clean], dst[clean], None, ws, route)


# ---- structural limits ----
LIMIT_H = (1, 64, 65)
SCAN_SIZES = (256, 257, 513)


@functools.lru_cache(maxsize=None)
def few_case(n_keep):
    """"a80" with only its first ``n_keep`` clean rows allowed: (src, dst, ok)."""
    src, dst, _, _, _, _, _, clean = case("a80")
    ok = np.zeros(len(src), bool)
    ok[np.nonzero(clean)[0][:n_keep]] = True
    return src, dst, ok


@functools.lru_cache(maxsize=None)
def collinear_case():
    """80 rows whose src lies on the line (x, x / 2 + 1 / 4, 1 - x / 4) at x = (j - 40) / 64 -- exact in binary: every cross product
    is exactly zero -- against "a80"'s dst: (src, dst)."""
    x = (np.arange(80) - 40) / 64.0
    src = np.stack([x, 0.5 * x + 0.25, 1.0 - 0.25 * x], axis=1)
    return src, case("a80")[1]


def interleave_nan(src, dst, ok=None, every=3):
    """The rows with a NaN row, forbidden by ok, put in front of every ``every``-th: (src', dst', ok', position of each old row)."""
    n = len(src)
    pos = np.arange(n) + (np.arange(n) + every - 1) // every
    m = pos[-1] + 1
    s2, d2, o2 = np.full((m, 3), np.nan), np.full((m, 3), np.nan), np.zeros(m, bool)
    s2[pos], d2[pos], o2[pos] = src, dst, True if ok is None else ok
    return s2, d2, o2, pos


@functools.lru_cache(maxsize=None)
def scan_case(n):
    """n rows of the construction (its own scene) under an ok mask: a seeded half of every row, the whole second chunk of 256
    forbidden where there is a third, the rows past the last full chunk allowed: (src, dst, ok)."""
    src, dst, _ = correspondences(n, SCALE)
    ok = np.random.default_rng(13).random(n) < 0.5
    if n > 512:
        ok[256:512] = False
    ok[256 * (n // 256):] = True
    ok.setflags(write=False)
    return src, dst, ok


@functools.lru_cache(maxsize=None)
def scan_reference(n, route="horn"):
    src, dst, ok = scan_case(n)
    return AR.align_robust(src, dst, THRESHOLD * SCALE, ok, True, 64, 1, 2, route)


MAX_HYP = RC.MAX_HYP


def max_hyp_sample():
    return RC.max_hyp_sample()


@functools.lru_cache(maxsize=None)
def max_hyp_reference(route="horn"):
    """(h, counts, guard, pivot) of "a80" at the h of max_hyp_sample()."""
    src, dst, _, ws, thr, _, seed, _ = case("a80")
    hs = max_hyp_sample()
    return (hs,) + AR.hypothesis_counts(src, dst, thr, seed, hs, ws, route)


REFIT_COUNTS = (0, 1, 16)
REFIT_THRESHOLD = 2.5e-3 * SCALE  # "a80" at 2.5 sigma: the inlier sets move between refits


@functools.lru_cache(maxsize=None)
def refit_reference(n_refit, route="horn"):
    src, dst, ok, ws, _, H, seed, _ = case("a80")
    return AR.align_robust(src, dst, REFIT_THRESHOLD, ok, ws, H, seed, n_refit, route)


# ---- control points ----
CONTROL_SCALE, N_CONTROL, N_WRONG = 3.0, 40, 12


def control_points(sc, point_ok, seed=17):
    """(ids, xyz, wrong): N_CONTROL of the points ``point_ok`` marks, surveyed in the ground-truth frame scaled by CONTROL_SCALE;
    N_WRONG of them with coordinates drawn uniformly from the box of all surveyed positions."""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(np.nonzero(point_ok)[0], N_CONTROL, replace=False))
    world = CONTROL_SCALE * sc.X_gt
    xyz = world[ids].copy()
    wrong = np.zeros(N_CONTROL, bool)
    wrong[rng.choice(N_CONTROL, N_WRONG, replace=False)] = True
    lo, hi = world.min(axis=0), world.max(axis=0)
    xyz[wrong] = lo + (hi - lo) * rng.random((N_WRONG, 3))
    return ids, xyz, wrong
