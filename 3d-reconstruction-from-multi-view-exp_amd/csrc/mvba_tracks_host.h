// The host logic of mvba_build_tracks (mvba_tracks.h), once: its argument checks, the check of the keypoint offsets and of the
// edge ids, the rule that classifies a component of the match graph by its size -- the one function the kernels use too --
// and the two sizes its launches share with the matcher's (mvba_match_host.h): the grid of a one-thread-per-item kernel and
// the block of the scan.  No HIP call in it: csrc/host_check.cpp runs it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#include "mvba_common.h"

#if defined(__HIP__)
#define TRK_HD __host__ __device__ __forceinline__
#else
#define TRK_HD inline
#endif

namespace mvba {

// counts [TRK_N_COUNTS] of mvba_build_tracks, in this order (include/mvba.h)
enum {
  TRK_C_TRACKS = 0, TRK_C_OBS, TRK_C_COMPONENTS, TRK_C_SHORT, TRK_C_CONFLICT, TRK_C_CONFLICT_NODES, TRK_C_OVERSIZE,
  TRK_C_OVERSIZE_NODES, TRK_C_SINGLETONS, TRK_C_ROUNDS, TRK_N_COUNTS
};
// node_track below 0
enum { TRK_UNMATCHED = -1, TRK_TOO_SHORT = -2, TRK_DROPPED = -3 };

constexpr int TRK_SCAN_ITEMS = 4;           // consecutive items per thread of k_tracks_scan_blocks
constexpr int TRK_SCAN_BLOCK = 256 * TRK_SCAN_ITEMS;

// the workgroups of 256 threads for n items, one at least (a kernel of these headers with nothing to do still starts)
inline unsigned trk_grid(long long n) { return (unsigned)std::max<long long>(1, (n + 255) / 256); }

// A component of `size` nodes (>= 1).  Singleton: no match at all.  Short: fewer nodes than a track must have.  Oversize: more
// nodes than images, so two of them lie in one image whatever they are -- dropped without being laid out.  Candidate: laid
// out, sorted, and kept unless two of its nodes share an image.  The first rule that holds decides.
enum { TRK_SINGLETON = 0, TRK_SHORT = 1, TRK_OVERSIZE = 2, TRK_CANDIDATE = 3 };
TRK_HD int tracks_classify(int size, int min_length, int n_images) {
  return size <= 1 ? TRK_SINGLETON : (size < min_length ? TRK_SHORT : (size > n_images ? TRK_OVERSIZE : TRK_CANDIDATE));
}

// kp_ptr [n_images + 1]: ascending from 0, below 2^31 nodes in all
inline int tracks_check_kp_ptr(int32_t n_images, const int64_t *kp_ptr) {
  if (n_images < 1) return fail(MVBA_ERR_BADARG, "n_images = " + std::to_string(n_images) + " must be at least 1");
  if (kp_ptr[0] != 0) return fail(MVBA_ERR_BADARG, "kp_ptr[0] = " + std::to_string(kp_ptr[0]) + " must be 0");
  for (int32_t i = 0; i < n_images; ++i)
    if (kp_ptr[i + 1] < kp_ptr[i])
      return fail(MVBA_ERR_BADARG, "kp_ptr is not ascending: kp_ptr[" + std::to_string(i + 1) + "] = " + std::to_string(kp_ptr[i + 1]) + " after " +
                                       std::to_string(kp_ptr[i]));
  if (kp_ptr[n_images] >= (1LL << 31))
    return fail(MVBA_ERR_BADARG, "n_nodes = kp_ptr[n_images] = " + std::to_string(kp_ptr[n_images]) + " must be < 2^31");
  return MVBA_OK;
}

// Everything mvba_build_tracks checks before it touches the device, in the order of its arguments' dependencies: the
// pointers (by name and position), the sizes, kp_ptr, then every edge id.
inline int tracks_check_args(int32_t n_images, const int64_t *kp_ptr, const double *kp_xy, const int32_t *edges, int64_t n_edges,
                             int32_t min_length, const int64_t *pt_ptr, const int32_t *cam_idx, const int32_t *obs_node, const double *xy,
                             const int32_t *node_track, const int64_t *counts) {
  if (!kp_ptr) return fail(MVBA_ERR_BADARG, "null argument: kp_ptr (argument 2)");
  if (!pt_ptr) return fail(MVBA_ERR_BADARG, "null argument: pt_ptr (argument 8)");
  if (!cam_idx) return fail(MVBA_ERR_BADARG, "null argument: cam_idx (argument 9)");
  if (!obs_node) return fail(MVBA_ERR_BADARG, "null argument: obs_node (argument 10)");
  if (!node_track) return fail(MVBA_ERR_BADARG, "null argument: node_track (argument 12)");
  if (!counts) return fail(MVBA_ERR_BADARG, "null argument: counts (argument 13)");
  if (xy && !kp_xy) return fail(MVBA_ERR_BADARG, "null argument: kp_xy (argument 3) with an xy to fill");
  if (n_edges < 0) return fail(MVBA_ERR_BADARG, "n_edges = " + std::to_string(n_edges) + ": negative size");
  if (n_edges > 0 && !edges) return fail(MVBA_ERR_BADARG, "null argument: edges (argument 4) with n_edges = " + std::to_string(n_edges));
  if (min_length < 2) return fail(MVBA_ERR_BADARG, "min_length = " + std::to_string(min_length) + " must be at least 2");
  if (int rc = tracks_check_kp_ptr(n_images, kp_ptr)) return rc;
  const int64_t n_nodes = kp_ptr[n_images];
  uint32_t worst = 0;  // one pass without a branch (a negative id is a large unsigned one); the search below runs only to report
  for (int64_t e = 0; e < 2 * n_edges; ++e) worst = worst > (uint32_t)edges[e] ? worst : (uint32_t)edges[e];
  if (n_edges == 0 || (int64_t)worst < n_nodes) return MVBA_OK;
  for (int64_t e = 0; e < 2 * n_edges; ++e)
    if (edges[e] < 0 || edges[e] >= n_nodes)
      return fail(MVBA_ERR_BADARG, "edges[" + std::to_string(e / 2) + "][" + std::to_string(e % 2) + "] = " + std::to_string(edges[e]) +
                                       ": node id out of range, n_nodes = " + std::to_string(n_nodes));
  return MVBA_OK;
}

}  // namespace mvba
