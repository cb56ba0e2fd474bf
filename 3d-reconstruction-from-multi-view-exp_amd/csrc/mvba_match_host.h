// The host logic of mvba_match_descriptors (mvba_match.h), once: its argument checks, the rule that cuts the pair list into
// chunks, the plan of a call (match_plan: the cuts and the size of every buffer), the block lists and offset tables of a chunk
// (match_chunk_lists), and the two pieces of arithmetic the kernels share with the host -- the squared ratio and the ratio
// test itself.  No HIP call in it: csrc/host_check.cpp runs it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "mvba_common.h"
#include "mvba_tracks_host.h"  // TRK_SCAN_BLOCK: the matches are compacted by the track builder's scan

#if defined(__HIP__)
#define MATCH_HD __host__ __device__ __forceinline__
#else
#define MATCH_HD inline
#endif

// MATCH_TQ queries [q0, q0 + nq) (node ids) of one directed job against the candidates [c0, c0 + nc); results at out0 + local
// query.  (In the unnamed namespace of mvba_match.h's kernels: the symbol of k_match_nn carries the name of this type.)
namespace {
struct MatchBlock {
  int q0, nq, c0, nc, out0;
};
}  // namespace

namespace mvba {

// counts [MATCH_N_COUNTS] of mvba_match_descriptors, in this order (include/mvba.h)
enum { MATCH_C_MATCHES = 0, MATCH_C_QUERIES, MATCH_C_NO_CANDIDATE, MATCH_C_FAR, MATCH_C_AMBIGUOUS, MATCH_C_NOT_MUTUAL, MATCH_N_COUNTS };
// what became of a query: 0 matched, else the first rule that held (its count is counts[1 + code])
enum { MATCH_KEPT = 0, MATCH_NO_CANDIDATE = 1, MATCH_FAR = 2, MATCH_AMBIGUOUS = 3, MATCH_NOT_MUTUAL = 4 };

constexpr int MATCH_TQ = 128;     // queries per workgroup: 4 waves x the 32 columns of an MFMA tile
constexpr int MATCH_TC = 128;     // candidates per LDS tile: 4 row blocks of an MFMA tile
constexpr int MATCH_KSTEP = 32;   // bytes of a descriptor per v_mfma_i32_32x32x32_i8
constexpr int MATCH_DIM_MAX = 512;  // 512 * 255^2 < 2^31, and so is every partial sum of the expansion
constexpr int64_t MATCH_CHUNK_QUERIES = 1LL << 22;  // queries (both directions) of the pairs answered together

// the squared ratio, rounded once, in double
inline double match_ratio2(double ratio) { return ratio * ratio; }

// Rule 3 on two exact integers (second2 < 0: there is no second).  One multiply and one compare: nothing to contract.
MATCH_HD bool match_ambiguous(int32_t best2, int32_t second2, double r2) {
  if (second2 < 0) return true;
  const double rhs = r2 * (double)second2;
  return !((double)best2 < rhs);
}

// Everything mvba_match_descriptors checks before it touches the device.  *n_queries: the sum of the query images' keypoint
// counts over the pairs (Q of the header).
inline int match_check_args(int32_t n_images, const int64_t *kp_ptr, const uint8_t *desc, int32_t dim, const int32_t *pairs, int32_t n_pairs,
                            double ratio, const int64_t *match_ptr, const int32_t *kp_pairs, const int32_t *dist2, const int64_t *counts,
                            int64_t *n_queries) {
  if (!kp_ptr) return fail(MVBA_ERR_BADARG, "null argument: kp_ptr (argument 2)");
  if (!match_ptr) return fail(MVBA_ERR_BADARG, "null argument: match_ptr (argument 10)");
  if (!kp_pairs) return fail(MVBA_ERR_BADARG, "null argument: kp_pairs (argument 11)");
  if (!dist2) return fail(MVBA_ERR_BADARG, "null argument: dist2 (argument 12)");
  if (!counts) return fail(MVBA_ERR_BADARG, "null argument: counts (argument 16)");
  if (n_pairs < 0) return fail(MVBA_ERR_BADARG, "n_pairs = " + std::to_string(n_pairs) + ": negative size");
  if (n_pairs > 0 && !pairs) return fail(MVBA_ERR_BADARG, "null argument: pairs (argument 5) with n_pairs = " + std::to_string(n_pairs));
  if (n_images < 1) return fail(MVBA_ERR_BADARG, "n_images = " + std::to_string(n_images) + " must be at least 1");
  if (kp_ptr[0] != 0) return fail(MVBA_ERR_BADARG, "kp_ptr[0] = " + std::to_string(kp_ptr[0]) + " must be 0");
  for (int32_t i = 0; i < n_images; ++i)
    if (kp_ptr[i + 1] < kp_ptr[i])
      return fail(MVBA_ERR_BADARG, "kp_ptr is not ascending: kp_ptr[" + std::to_string(i + 1) + "] = " + std::to_string(kp_ptr[i + 1]) + " after " +
                                       std::to_string(kp_ptr[i]));
  if (kp_ptr[n_images] >= (1LL << 31))
    return fail(MVBA_ERR_BADARG, "n_nodes = kp_ptr[n_images] = " + std::to_string(kp_ptr[n_images]) + " must be < 2^31");
  if (kp_ptr[n_images] > 0 && !desc)
    return fail(MVBA_ERR_BADARG, "null argument: desc (argument 3) with " + std::to_string(kp_ptr[n_images]) + " keypoints");
  if (dim < 16 || dim > MATCH_DIM_MAX || dim % 16)
    return fail(MVBA_ERR_BADARG, "dim = " + std::to_string(dim) + " must be a multiple of 16 in 16 .. " + std::to_string(MATCH_DIM_MAX));
  if (!(ratio >= 0.0 && ratio <= 1.0)) return fail(MVBA_ERR_BADARG, "ratio = " + std::to_string(ratio) + " must be in (0, 1], or 0 for no ratio test");
  int64_t Q = 0;
  for (int32_t p = 0; p < n_pairs; ++p) {
    for (int e = 0; e < 2; ++e)
      if (pairs[2 * p + e] < 0 || pairs[2 * p + e] >= n_images)
        return fail(MVBA_ERR_BADARG, "pairs[" + std::to_string(p) + "][" + std::to_string(e) + "] = " + std::to_string(pairs[2 * p + e]) +
                                         ": image index out of range, n_images = " + std::to_string(n_images));
    if (pairs[2 * p] == pairs[2 * p + 1])
      return fail(MVBA_ERR_BADARG, "pairs[" + std::to_string(p) + "] = (" + std::to_string(pairs[2 * p]) + ", " + std::to_string(pairs[2 * p + 1]) +
                                       "): an image is not matched with itself");
    Q += kp_ptr[pairs[2 * p] + 1] - kp_ptr[pairs[2 * p]];
    if (Q >= (1LL << 31))
      return fail(MVBA_ERR_BADARG, "Q = " + std::to_string(Q) + " queries up to pair " + std::to_string(p) + ": the sum over the pairs must be < 2^31");
  }
  *n_queries = Q;
  return MVBA_OK;
}

// The end of the chunk that starts at pair p0: pairs are taken while the chunk's per-query rows -- one per query, and with
// `mutual` one per candidate for the reverse direction -- stay within `budget`; one pair at least, whatever its size.
inline int32_t match_chunk_end(const int64_t *kp_ptr, const int32_t *pairs, int32_t n_pairs, int32_t p0, bool mutual, int64_t budget) {
  int64_t rows = 0;
  int32_t p = p0;
  for (; p < n_pairs; ++p) {
    const int64_t nk = kp_ptr[pairs[2 * p] + 1] - kp_ptr[pairs[2 * p]], nl = kp_ptr[pairs[2 * p + 1] + 1] - kp_ptr[pairs[2 * p + 1]];
    const int64_t more = nk + (mutual ? nl : 0);
    if (p > p0 && rows + more > budget) break;
    rows += more;
  }
  return p;
}

// The chunks of a call -- chunk c answers the pairs cut[c] .. cut[c + 1] - 1, the cuts are match_chunk_end's -- and the largest
// of each buffer any of them needs: max_q queries, max_r reverse rows (0 without `mutual`) and max_p pairs of one chunk; from
// these the MatchBlocks of both lists together, the workgroups of k_match_decide and the blocks of the scan.  A job of nq
// queries has ceil(nq / MATCH_TQ) <= nq / MATCH_TQ + 1 blocks and a chunk 2 max_p jobs at most: hence max_blocks.
struct MatchPlan {
  std::vector<int32_t> cut{0};
  size_t max_q = 0, max_r = 0, max_p = 0, max_blocks = 0, max_dec = 0, max_sb = 0;
};

inline MatchPlan match_plan(const int64_t *kp_ptr, const int32_t *pairs, int32_t n_pairs, bool mutual, int64_t budget) {
  MatchPlan pl;
  while (pl.cut.back() < n_pairs) {
    const int32_t p0 = pl.cut.back(), p1 = match_chunk_end(kp_ptr, pairs, n_pairs, p0, mutual, budget);
    size_t q = 0, r = 0;
    for (int32_t p = p0; p < p1; ++p) {
      q += (size_t)(kp_ptr[pairs[2 * p] + 1] - kp_ptr[pairs[2 * p]]);
      r += (size_t)(kp_ptr[pairs[2 * p + 1] + 1] - kp_ptr[pairs[2 * p + 1]]);
    }
    pl.max_q = std::max(pl.max_q, q);
    pl.max_r = std::max(pl.max_r, mutual ? r : 0);
    pl.max_p = std::max(pl.max_p, (size_t)(p1 - p0));
    pl.cut.push_back(p1);
  }
  pl.max_blocks = (pl.max_q + pl.max_r) / MATCH_TQ + 2 * pl.max_p + 1;
  pl.max_dec = (pl.max_q + 255) / 256;
  pl.max_sb = (pl.max_q + TRK_SCAN_BLOCK - 1) / TRK_SCAN_BLOCK;
  return pl;
}

// What the pairs p0 .. p1 - 1 of one chunk ask of the device.  fwd: the blocks of the jobs (query image k, candidate image l)
// of its pairs (k, l), pair i's results from row qoff[i] on; rev (with `mutual`, else empty and roff all 0): those of (l, k),
// from row roff[i] on.  qoff, roff [P + 1]; ncand [P]: the candidates of a pair's queries; Qc = qoff[P]: the chunk's queries.
struct MatchLists {
  std::vector<MatchBlock> fwd, rev;
  std::vector<int> qoff, roff, ncand;
  int P = 0, Qc = 0;
};

inline void match_chunk_lists(const int64_t *kp_ptr, const int32_t *pairs, int32_t p0, int32_t p1, bool mutual, MatchLists &L) {
  auto add = [&](std::vector<MatchBlock> &blocks, int q, int c, int out) {  // the blocks of the job (q, c), its results from row `out` on
    const int q0 = (int)kp_ptr[q], nq = (int)(kp_ptr[q + 1] - kp_ptr[q]), c0 = (int)kp_ptr[c], nc = (int)(kp_ptr[c + 1] - kp_ptr[c]);
    for (int at = 0; at < nq; at += MATCH_TQ) blocks.push_back(MatchBlock{q0 + at, std::min(MATCH_TQ, nq - at), c0, nc, out + at});
  };
  const int P = L.P = p1 - p0;
  L.fwd.clear(); L.rev.clear();
  L.qoff.assign((size_t)P + 1, 0); L.roff.assign((size_t)P + 1, 0); L.ncand.assign((size_t)P, 0);
  for (int i = 0; i < P; ++i) {
    const int k = pairs[2 * (p0 + i)], l = pairs[2 * (p0 + i) + 1];
    add(L.fwd, k, l, L.qoff[i]);
    if (mutual) add(L.rev, l, k, L.roff[i]);
    L.qoff[i + 1] = L.qoff[i] + (int)(kp_ptr[k + 1] - kp_ptr[k]);
    L.roff[i + 1] = L.roff[i] + (mutual ? (int)(kp_ptr[l + 1] - kp_ptr[l]) : 0);
    L.ncand[i] = (int)(kp_ptr[l + 1] - kp_ptr[l]);
  }
  L.Qc = L.qoff[P];
}

}  // namespace mvba
