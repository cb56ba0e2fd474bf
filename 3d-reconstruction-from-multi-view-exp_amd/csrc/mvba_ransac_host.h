// The host logic of a RANSAC round, once: what mvba_two_view_robust, mvba_homography_robust, mvba_resect_robust,
// mvba_pose_robust and mvba_align_robust decide on plain integers between their kernels (mvba_ransac.h, mvba_resect_ransac.h,
// mvba_pose_ransac.h, mvba_align.h) -- the three decisions rs_pick, rs_accept and rs_stop, the loops over a tile's items
// around them (RsTile) and the choice between the two mask buffers (rs_current, rs_other: the kernels use it too) -- and the
// chunk list of the listed cameras (mvba_init.h's CamWork); the cyclic Jacobi the start headers share, and align_solve, the
// similarity fit of mvba_align.h from centred moments.  No HIP call in it: csrc/host_check.cpp runs it under the host
// sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "mvba_common.h"

#if defined(__HIP__)
#define RS_HD __host__ __device__  // a helper the kernels use too
#define RS_HD_INLINE __host__ __device__ __forceinline__
#else
#define RS_HD
#define RS_HD_INLINE inline
#endif

namespace mvba {

constexpr int RS_MAX_HYP = 65536;  // n_hypotheses
constexpr int RS_MAX_REFIT = 16;   // n_refit
enum { RS_CUR = 1, RS_ACTIVE = 2, RS_OK = 4 };  // per-item state: the current mask buffer, still refitting, status 0

// The two mask buffers of an item under its state: RS_CUR names the CURRENT one, the inlier set of the model the item keeps;
// a mask pass writes the OTHER one.  rs_pick hands an item out with RS_CUR set, so the first mask -- the best hypothesis's --
// goes to buffer 0; the toggle that follows makes it current.  A refit sums over the current buffer and masks into the other;
// rs_accept toggles if the refit is kept, and otherwise the current buffer stays what it was.  (T: const or not.)
template <class T>
RS_HD_INLINE T *rs_current(int st, T *inl0, T *inl1) {
  return (st & RS_CUR) ? inl1 : inl0;
}
template <class T>
RS_HD_INLINE T *rs_other(int st, T *inl0, T *inl1) {
  return (st & RS_CUR) ? inl0 : inl1;
}

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

// The rounds of one tile of items on the host, between the kernels: the pairs of robust_pairs, the cameras of
// robust_cameras, the one alignment of mvba_align_robust.  The caller runs the kernels and brings S2 [item][2] = (inlier
// count, sum of d^2) of each mask pass; the tile holds what the items keep and moves their state bits:
//   defaults, once per call;  per tile: pick -> the first mask -> first -> per refit (the fit, rs_stop where it fails, the
//   mask, accept) -> write.
struct RsTile {
  std::vector<int> st, best;   // per item: the status, the best hypothesis (-1: none)
  std::vector<long long> nin;  // the inliers of the model the item keeps
  std::vector<double> ssq;     // their sum of d^2
  int *state = nullptr;        // the items' states, the caller's array (robust_cameras keeps one over its whole list)
  const int *hc = nullptr;     // [cnt][H]: the counts pick went by
  int cnt = 0, H = 0, n_active = 0;

  explicit RsTile(int tile) : st((size_t)tile), best((size_t)tile), nin((size_t)tile), ssq((size_t)tile) {}

  // What a call writes before any work, for n items of H hypotheses: those of an item without observations, status 1.  n_item
  // is the output of the items' sizes (n_shared, n_usable); every pointer may be null.
  static void defaults(size_t n, int H, int32_t *status, int32_t *best, int32_t *hyp_count, int64_t *n_item, int64_t *n_inliers,
                       double *quality) {
    for (size_t g = 0; g < n; ++g) {
      if (quality) quality[2 * g] = quality[2 * g + 1] = NAN;
      if (n_item) n_item[g] = 0;
      if (n_inliers) n_inliers[g] = 0;
      if (best) best[g] = -1;
      if (status) status[g] = 1;
    }
    if (hyp_count) std::fill(hyp_count, hyp_count + n * (size_t)H, -1);
  }

  // rs_pick per item of a tile of cnt_ items (at most the tile the constructor was given): hyp_count [cnt_][H_] as the scoring
  // kernel left it, n_item the items' sizes, state_ where their states go
  void pick(int cnt_, int *state_, const int *hyp_count, int H_, const int *n_item, int n_min) {
    cnt = cnt_; state = state_; hc = hyp_count; H = H_; n_active = 0;
    for (int p = 0; p < cnt; ++p) {
      const RsPick k = rs_pick(hc + (size_t)p * H, H, n_item[p], n_min);
      st[p] = k.status;
      best[p] = k.best;
      state[p] = k.state;
    }
  }

  // After the first mask: the best hypothesis's inlier set becomes the current one of every item of status 0, and finish(p)
  // -> its status says whether the hypothesis is a model the item can keep (non-zero: the item is out, its state 0).  Returns
  // the number of items that go into the refits.
  template <class Finish>
  int first(const double *S2, Finish finish) {
    n_active = 0;
    for (int p = 0; p < cnt; ++p) {
      if (st[p]) continue;
      state[p] ^= RS_CUR;
      nin[p] = (long long)S2[2 * p];
      ssq[p] = S2[2 * p + 1];
      st[p] = finish(p);
      if (st[p]) state[p] = 0;
      else ++n_active;
    }
    return n_active;
  }

  // After the mask of refit r (from 0): rs_accept per active item; keep(p) for those whose refit becomes the kept model
  template <class Keep>
  void accept(int r, const double *S2, long long first_min, Keep keep) {
    for (int p = 0; p < cnt; ++p) {
      if (!(state[p] & RS_ACTIVE)) continue;
      const long long c = (long long)S2[2 * p];
      if (!rs_accept(c, nin[p], r, first_min, state[p], n_active)) continue;
      nin[p] = c;
      ssq[p] = S2[2 * p + 1];
      keep(p);
    }
  }

  // The tile's outputs, item p at g0 + p (every pointer may be null): status, best and the counts of every item; of an item of
  // status 0 also n_inliers and quality = (the RMS distance of its inliers, q1(p)).  q1 is called once per item of status 0,
  // wanted or not: it is where the caller writes the item's model.
  template <class Q1>
  void write(size_t g0, int32_t *status, int32_t *best_out, int32_t *hyp_count, int64_t *n_inliers, double *quality, Q1 q1) const {
    for (int p = 0; p < cnt; ++p) {
      const size_t g = g0 + p;
      if (status) status[g] = st[p];
      if (best_out) best_out[g] = best[p];
      if (hyp_count) std::copy(hc + (size_t)p * H, hc + (size_t)(p + 1) * H, hyp_count + g * H);
      if (st[p]) continue;
      const double q = q1(p);
      if (n_inliers) n_inliers[g] = nin[p];
      if (quality) {
        quality[2 * g] = sqrt(ssq[p] / (double)nin[p]);
        quality[2 * g + 1] = q;
      }
    }
  }
};

constexpr double INIT_REL_PIVOT = 1e-12;  // the relative pivot rule of mvba_covariance

// Eigen-decomposition of a symmetric N x N matrix by cyclic Jacobi (Rutishauser's rotations): A -> diagonal, V -> the
// eigenvectors in its columns.  Every index is a compile-time constant once the loops are unrolled: on the device the
// order-4 instance lives in registers (the form of mvsvd.hip's per-point solver).  A rotation is skipped once a_pq no
// longer changes either diagonal entry in floating point.
template <int N>
RS_HD_INLINE void sym_eig_jacobi(double (&A)[N][N], double (&V)[N][N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool any = false;
#pragma unroll
    for (int p = 0; p < N - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
        const double g = fabs(apq);
        if (!(g > 0.0) || (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq))) {
          A[p][q] = A[q][p] = 0.0;
          continue;
        }
        any = true;
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
        A[p][p] = app - t * apq;
        A[q][q] = aqq + t * apq;
        A[p][q] = A[q][p] = 0.0;
#pragma unroll
        for (int r = 0; r < N; ++r) {
          if (r != p && r != q) {
            const double arp = A[r][p], arq = A[r][q];
            A[r][p] = A[p][r] = arp - s * (arq + tau * arp);
            A[r][q] = A[q][r] = arq + s * (arp - tau * arq);
          }
          const double vrp = V[r][p], vrq = V[r][q];
          V[r][p] = vrp - s * (vrq + tau * vrp);
          V[r][q] = vrq + s * (vrp - tau * vrq);
        }
      }
    if (!any) break;
  }
}

// smallest, second-smallest and largest eigenvalue after sym_eig_jacobi, and the column of the smallest
template <int N>
RS_HD_INLINE void eig_extremes(const double (&A)[N][N], const double (&V)[N][N], double &l1, double &l2, double &lmax, double (&v)[N]) {
  int best = 0;
  l1 = A[0][0];
  lmax = A[0][0];
#pragma unroll
  for (int i = 1; i < N; ++i) {
    if (A[i][i] < l1) { l1 = A[i][i]; best = i; }
    lmax = fmax(lmax, A[i][i]);
  }
  l2 = HUGE_VAL;
#pragma unroll
  for (int i = 0; i < N; ++i)
    if (i != best) l2 = fmin(l2, A[i][i]);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double x = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) x = j == best ? V[i][j] : x;  // (selects: a run-time column index would put V into scratch)
    v[i] = x;
  }
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

// Absolute orientation, y ~ s Q x + tau, from centred moments (Horn's quaternion form): mx and my are the two centroids, mom =
// (sum |x_c|^2, sum |y_c|^2, C row-major with C[a][b] = sum y_c[a] x_c[b]).  q = the eigenvector of the largest eigenvalue of
// Horn's symmetric 4 x 4 matrix of C, by sym_eig_jacobi<4>: a unit quaternion is a proper rotation, there is no reflection to
// repair.  s = sum y_c . (Q x_c) / sum |x_c|^2 (1 unless with_scale), tau = my - s Q mx.  sim13 = (s, Q row-major, tau); *gap =
// (l1 - l2) / l1 of the two largest eigenvalues.  Returns 0, or 2 (sim13 NaN) where a moment is not finite, sum |x_c|^2 or
// sum |y_c|^2 is not positive, l1 is not positive, the gap fails the relative pivot rule -- the source or the target lies on a
// line: the rotation about it is free -- or the result is not finite or s is not positive.  In registers on the device: every
// index is a compile-time constant.
RS_HD_INLINE int align_solve(const double (&mx)[3], const double (&my)[3], const double (&mom)[11], bool with_scale, double (&sim13)[13],
                             double &gap) {
  gap = NAN;
#pragma unroll
  for (int e = 0; e < 13; ++e) sim13[e] = NAN;
  bool fin = mom[0] > 0.0 && mom[1] > 0.0;  // (NaN fails)
#pragma unroll
  for (int e = 0; e < 11; ++e) fin = fin && fabs(mom[e]) < HUGE_VAL;
  if (!fin) return 2;
  // S[a][b] = sum x_c[a] y_c[b] = C[b][a]; the matrix is negated so that eig_extremes' smallest is Horn's largest
  const double Sxx = mom[2], Sxy = mom[5], Sxz = mom[8], Syx = mom[3], Syy = mom[6], Syz = mom[9], Szx = mom[4], Szy = mom[7], Szz = mom[10];
  double A[4][4], V[4][4];
  A[0][0] = -(Sxx + Syy + Szz);
  A[1][1] = -(Sxx - Syy - Szz);
  A[2][2] = -(-Sxx + Syy - Szz);
  A[3][3] = -(-Sxx - Syy + Szz);
  A[0][1] = A[1][0] = -(Syz - Szy);
  A[0][2] = A[2][0] = -(Szx - Sxz);
  A[0][3] = A[3][0] = -(Sxy - Syx);
  A[1][2] = A[2][1] = -(Sxy + Syx);
  A[1][3] = A[3][1] = -(Szx + Sxz);
  A[2][3] = A[3][2] = -(Syz + Szy);
  sym_eig_jacobi<4>(A, V);
  double l1, l2, lmax, q[4];
  eig_extremes<4>(A, V, l1, l2, lmax, q);
  l1 = -l1;
  l2 = -l2;
  if (!(l1 > 0.0)) return 2;
  gap = (l1 - l2) / l1;
  if (!(gap > INIT_REL_PIVOT)) return 2;
  const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
  const double Q[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z),       2.0 * (x * z + w * y),
                       2.0 * (x * y + w * z),       1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                       2.0 * (x * z - w * y),       2.0 * (y * z + w * x),       1.0 - 2.0 * (x * x + y * y)};
  double s = 1.0;
  if (with_scale) {
    double num = 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) num += Q[e] * mom[2 + e];
    s = num / mom[0];
  }
  double out[13];
  out[0] = s;
#pragma unroll
  for (int e = 0; e < 9; ++e) out[1 + e] = Q[e];
#pragma unroll
  for (int a = 0; a < 3; ++a) out[10 + a] = my[a] - s * (Q[3 * a] * mx[0] + Q[3 * a + 1] * mx[1] + Q[3 * a + 2] * mx[2]);
  fin = s > 0.0;
#pragma unroll
  for (int e = 0; e < 13; ++e) fin = fin && fabs(out[e]) < HUGE_VAL;
  if (!fin) return 2;
#pragma unroll
  for (int e = 0; e < 13; ++e) sim13[e] = out[e];
  return 0;
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
