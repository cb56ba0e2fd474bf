// The host logic of a RANSAC round, once: what mvba_two_view_robust, mvba_resect_robust and mvba_pose_robust decide on plain
// integers between their kernels (mvba_ransac.h, mvba_resect_ransac.h, mvba_pose_ransac.h), and the chunk list of the
// listed cameras (mvba_init.h's CamWork).  No HIP call in it: csrc/host_check.cpp runs it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "mvba_common.h"

#if defined(__HIP__)
#define RS_HD __host__ __device__  // a helper the kernels use too
#else
#define RS_HD
#endif

namespace mvba {

constexpr int RS_MAX_HYP = 65536;  // n_hypotheses
constexpr int RS_MAX_REFIT = 16;   // n_refit
enum { RS_CUR = 1, RS_ACTIVE = 2, RS_OK = 4 };  // per-item state: the current mask buffer, still refitting, status 0

inline int rs_check_search(double threshold, int32_t n_hypotheses, int max_hyp = RS_MAX_HYP) {
  if (!std::isfinite(threshold) || !(threshold > 0.0))
    return fail(MVBA_ERR_BADARG, "threshold = " + std::to_string(threshold) + " must be finite and > 0");
  if (n_hypotheses < 1 || n_hypotheses > max_hyp)
    return fail(MVBA_ERR_BADARG, "n_hypotheses = " + std::to_string(n_hypotheses) + " must be in 1 .. " + std::to_string(max_hyp));
  return MVBA_OK;
}
inline int rs_check_refit(int32_t n_refit) {
  if (n_refit < 0 || n_refit > RS_MAX_REFIT)
    return fail(MVBA_ERR_BADARG, "n_refit = " + std::to_string(n_refit) + " must be in 0 .. " + std::to_string(RS_MAX_REFIT));
  return MVBA_OK;
}

// a list of cameras: in range, or NULL for every camera
inline int check_camera_list(const int32_t *cameras, int32_t n_cameras, int32_t m) {
  if (!cameras && n_cameras != m)
    return fail(MVBA_ERR_BADARG, "cameras = NULL lists every camera: n_cameras = " + std::to_string(n_cameras) + " must be n_images = " + std::to_string(m));
  for (int32_t c = 0; cameras && c < n_cameras; ++c)
    if (cameras[c] < 0 || cameras[c] >= m)
      return fail(MVBA_ERR_BADARG, "cameras[" + std::to_string(c) + "] = " + std::to_string(cameras[c]) + ": camera index out of range, n_images = " + std::to_string(m));
  return MVBA_OK;
}

// The best hypothesis of an item (a pair, a camera) of n_item observations from its H counts, for a model that needs n_min:
// status 1: the item is below n_min, 2: every hypothesis is degenerate (count -1), 4: the best count is below n_min, else 0.
struct RsPick {
  int best, status, state;
};
inline RsPick rs_pick(const int *count, int H, long long n_item, int n_min) {
  int b = 0;  // arg-max: the largest count, the lowest h on ties
  for (int h = 1; h < H; ++h)
    if (count[h] > count[b]) b = h;
  RsPick r;
  r.status = n_item < n_min ? 1 : (count[b] < 0 ? 2 : (count[b] < n_min ? 4 : 0));
  r.best = count[b] < 0 ? -1 : b;  // (status 1 and 2: every count is -1)
  r.state = r.status == 0 ? (RS_OK | RS_ACTIVE | RS_CUR) : 0;  // (the first mask goes into buffer 0)
  return r;
}

// an item's refit has failed, or its inlier set has shrunk: it keeps what it has
inline void rs_stop(int &state, int &n_active) {
  state &= ~RS_ACTIVE;
  --n_active;
}

// The accept rule of refit r (from 0) with `count` inliers against the `kept` ones: kept while the set does not shrink; a
// model with a first_min > 0 holds its first refit to that instead.  true: the new mask becomes the current one.
inline bool rs_accept(long long count, long long kept, int r, long long first_min, int &state, int &n_active) {
  if (count >= (r == 0 && first_min > 0 ? first_min : kept)) {
    state ^= RS_CUR;
    return true;
  }
  rs_stop(state, n_active);
  return false;
}

// The homography's host arithmetic between the kernels of mvba_homography_robust (row-major 3 x 3 matrices).
// adj(M): M adj(M) = det(M) I -- the inverse up to scale, which is all a homography needs
RS_HD inline void hg_adjugate(const double *m, double *a) {
  a[0] = m[4] * m[8] - m[5] * m[7]; a[1] = m[2] * m[7] - m[1] * m[8]; a[2] = m[1] * m[5] - m[2] * m[4];
  a[3] = m[5] * m[6] - m[3] * m[8]; a[4] = m[0] * m[8] - m[2] * m[6]; a[5] = m[2] * m[3] - m[0] * m[5];
  a[6] = m[3] * m[7] - m[4] * m[6]; a[7] = m[1] * m[6] - m[0] * m[7]; a[8] = m[0] * m[4] - m[1] * m[3];
}
// the form a matrix is returned in: Frobenius norm 1, the largest-magnitude entry (the first of equals) positive.  false if
// an entry is not finite or the matrix is zero (it is left as it is then).
inline bool hg_unit(double *m) {
  double nrm = 0.0, big = 0.0;
  for (int j = 0; j < 9; ++j) {
    nrm += m[j] * m[j];
    if (std::fabs(m[j]) > std::fabs(big)) big = m[j];
  }
  if (!std::isfinite(nrm) || !(nrm > 0.0)) return false;
  const double sc = (big < 0.0 ? -1.0 : 1.0) / std::sqrt(nrm);
  for (int j = 0; j < 9; ++j) m[j] *= sc;
  return true;
}
// The two matrices the inlier test reads, out of H (x_l ~ H x_k): the test asks for a positive third coordinate, so the sign
// matters.  m0 = +-H and m1 = +-adj(H), each with the sign that makes the third coordinate positive at the centroid of the
// points it is applied to -- (ckx, cky) in k, (clx, cly) in l: nm[0], nm[1], nm[3], nm[4] of the fit's TV_NORM record.
inline void hg_mask_parts(const double *H, const double *nm, double *m0, double *m1) {
  hg_adjugate(H, m1);
  const double wk = H[6] * nm[0] + H[7] * nm[1] + H[8], wl = m1[6] * nm[3] + m1[7] * nm[4] + m1[8];
  for (int j = 0; j < 9; ++j) {
    m0[j] = wk < 0.0 ? -H[j] : H[j];
    if (wl < 0.0) m1[j] = -m1[j];
  }
}

// the four phases of a robust call, in milliseconds
struct RsLaps {
  double upload = 0.0, score = 0.0, refit = 0.0, other = 0.0;
  void write(double *timings_ms) const {
    if (!timings_ms) return;
    timings_ms[0] = upload;
    timings_ms[1] = score;
    timings_ms[2] = refit;
    timings_ms[3] = other;
  }
};

// The listed cameras' runs of a camera-major list (cam_ptr: the runs of all cameras; cameras == nullptr: list position =
// camera) and their chunks of `chunk` observations; a listed camera's bytes in the mask buffers start at its offset in the
// concatenation of the listed runs (a camera listed twice has two).
struct CamChunks {
  std::vector<int> cams, lc_n, lc_ch, ch_cam, ch_cnt;
  std::vector<long long> lc_start, lc_mask, ch_start, ch_mask;
  long long n_mask = 0;
  int n_ch = 0;

  int build(const long long *cam_ptr, const int32_t *cameras, int nl, int chunk, int64_t *n_usable) {
    cams.resize((size_t)nl); lc_n.resize((size_t)nl); lc_start.resize((size_t)nl); lc_mask.resize((size_t)nl);
    lc_ch.assign((size_t)nl + 1, 0);
    for (int c = 0; c < nl; ++c) {
      const int k = cameras ? cameras[c] : c;
      const long long n = cam_ptr[k + 1] - cam_ptr[k];
      if (n >= (1LL << 31)) return fail(MVBA_ERR_BADARG, "camera " + std::to_string(k) + " has " + std::to_string(n) + " usable observations: must be < 2^31");
      cams[c] = k;
      lc_n[c] = (int)n;
      lc_start[c] = cam_ptr[k];
      lc_mask[c] = n_mask;
      if (n_usable) n_usable[c] = n;
      for (long long s = 0; s < n; s += chunk) {
        ch_cam.push_back(c);
        ch_start.push_back(cam_ptr[k] + s);
        ch_mask.push_back(n_mask + s);
        ch_cnt.push_back((int)std::min<long long>(chunk, n - s));
      }
      n_mask += n;
      if (ch_cam.size() > (size_t)0x7fffffff) return fail(MVBA_ERR_BADARG, "too many chunks of 256 observations over the listed cameras");
      lc_ch[c + 1] = (int)ch_cam.size();
    }
    n_ch = (int)ch_cam.size();
    return MVBA_OK;
  }
};

}  // namespace mvba
