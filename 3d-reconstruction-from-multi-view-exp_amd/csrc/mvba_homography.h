// Planar scenes (mvba_homography_robust, mvba_homography_sample): 4-point RANSAC for the homography of two views -- kernels
// and host code, gfx950.
//
// Included by mvba.hip after mvba_ransac.h: the call IS mvba_ransac.h's robust_pairs -- its compaction, normalisation, scoring,
// mask, refit, gather and scatter kernels, its host loop and its sample_entry -- with the model below in place of the
// fundamental matrix:
// HomogModel, the inlier test of k_ransac_score and k_ransac_mask; k_homog_hyp, the hypothesis kernel; tv_pass mode 4, the
// refit's moments (mvba_twoview.h); homography_solve_pair (mvba_twoview.h) and hg_mask_parts (mvba_ransac_host.h), the host
// steps.  Nothing here runs on the LM path.  
//
// A hypothesis is two 3 x 3 matrices, H (k -> l) and H^-1 up to scale (l -> k): part 0 and part 1 of the hypothesis array.  A
// point is an inlier if BOTH transfers land within the threshold with a positive third coordinate, tested without a division.
// The sign of a matrix therefore matters: each is given the sign that makes the third coordinate positive at the centroid of
// the points it is applied to (the origin of the normalised coordinates: the entry [2][2] of the normalised matrix).

namespace {

struct HomogModel {
  static constexpr int PARTS = 2, MIN = 4;
  // (u, v, w) = M (x, y, 1): the squared distance of (u / w, v / w) from (tx, ty), times w^2
  static __device__ __forceinline__ double transfer(const double *M, double x, double y, double tx, double ty, double &w) {
    const double u = M[0] * x + M[1] * y + M[2], v = M[3] * x + M[4] * y + M[5];
    w = M[6] * x + M[7] * y + M[8];
    const double eu = u - tx * w, ev = v - ty * w;
    return eu * eu + ev * ev;
  }
  // The test: both transfers within the threshold with a positive third coordinate, decided WITHOUT a division -- w > 0 and
  // (u - x w)^2 + (v - y w)^2 <= thr^2 w^2 each way (NaN: fails).  The scoring kernel runs this and nothing else of the model.
  static __device__ __forceinline__ bool inlier(const double *Hf, const double *Hb, double xk, double yk, double xl, double yl, double thr2) {
    double wf, wb;
    const double af = transfer(Hf, xk, yk, xl, yl, wf), ab = transfer(Hb, xl, yl, xk, yk, wb);
    return wf > 0.0 && af <= thr2 * (wf * wf) && wb > 0.0 && ab <= thr2 * (wb * wb);
  }
  // The mask pass: the mean of the two squared transfer distances (two divisions per point, once per refit), or infinity for
  // a point that fails the test above.  The mean of two terms that are each <= thr^2 is <= thr^2 up to the rounding of the
  // divisions, which the clamp removes: the caller's comparison with thr^2 passes exactly the points that pass inlier().
  static __device__ __forceinline__ double dist2(const double *Hf, const double *Hb, double xk, double yk, double xl, double yl, double thr2) {
    double wf, wb;
    const double af = transfer(Hf, xk, yk, xl, yl, wf), ab = transfer(Hb, xl, yl, xk, yk, wb);
    const double wf2 = wf * wf, wb2 = wb * wb;
    const bool in = wf > 0.0 && af <= thr2 * wf2 && wb > 0.0 && ab <= thr2 * wb2;
    return in ? fmin(0.5 * (af / wf2 + ab / wb2), thr2) : HUGE_VAL;
  }
};

// det [(a, 1) (b, 1) (c, 1)], the points as columns: twice the signed area of the triangle
__device__ __forceinline__ double hg_det(const double (&a)[2], const double (&b)[2], const double (&c)[2]) {
  return a[0] * (b[1] - c[1]) - b[0] * (a[1] - c[1]) + c[0] * (a[1] - b[1]);
}

// One image's half of the 4-point solution: B = [l1 p1, l2 p2, l3 p3] (row-major, the points (x, y, 1) as columns) with
// [p1 p2 p3] l = p4 solved by the adjugate -- Cramer's rule, l_i = the determinant with p4 in column i; the common factor
// 1 / det [p1 p2 p3] is left out: a homography has no scale.  B maps the canonical frame (e1, e2, e3, e1 + e2 + e3) onto the
// four points.  false if any of the four triples is collinear by the pivot rule.
__device__ __forceinline__ bool hg_basis(const double (&p)[4][2], double (&B)[9]) {
  double nr[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) nr[c] = sqrt(p[c][0] * p[c][0] + p[c][1] * p[c][1] + 1.0);
  const double d123 = hg_det(p[0], p[1], p[2]), l1 = hg_det(p[3], p[1], p[2]), l2 = hg_det(p[0], p[3], p[2]), l3 = hg_det(p[0], p[1], p[3]);
  B[0] = l1 * p[0][0]; B[1] = l2 * p[1][0]; B[2] = l3 * p[2][0];
  B[3] = l1 * p[0][1]; B[4] = l2 * p[1][1]; B[5] = l3 * p[2][1];
  B[6] = l1; B[7] = l2; B[8] = l3;
  return fabs(d123) > INIT_REL_PIVOT * (nr[0] * nr[1] * nr[2]) && fabs(l1) > INIT_REL_PIVOT * (nr[3] * nr[1] * nr[2]) &&
         fabs(l2) > INIT_REL_PIVOT * (nr[0] * nr[3] * nr[2]) && fabs(l3) > INIT_REL_PIVOT * (nr[0] * nr[1] * nr[3]);
}

// out = +-A adj(B), the sign that makes out[8] positive
__device__ __forceinline__ void hg_map(const double (&A)[9], const double (&B)[9], double (&out)[9]) {
  double a[9];
  hg_adjugate(B, a);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * i + j] = A[3 * i] * a[j] + A[3 * i + 1] * a[3 + j] + A[3 * i + 2] * a[6 + j];
  if (out[8] < 0.0) {
#pragma unroll
    for (int e = 0; e < 9; ++e) out[e] = -out[e];
  }
}

// One thread per hypothesis, in registers alone (no LDS, no scratch, no iteration): the first four draws of rs_sample, the
// closed-form homography of the four normalised correspondences, H^ = B_l adj(B_k) and H^^-1 ~ B_k adj(B_l), denormalised into
// part 0 (H) and part 1 (H^-1) of hyp; hyp_count = 0, or -1 (and NaN matrices) if degenerate.
__global__ __launch_bounds__(RS_HYP_BLOCK) void k_homog_hyp(long long stride, int H, unsigned long long seed, const int *__restrict__ pairs,
                                                            const int *__restrict__ ntot, const double4 *__restrict__ comp,
                                                            const double *__restrict__ norm, double *__restrict__ hyp, int *__restrict__ hyp_count) {
  const int p = blockIdx.y, h = blockIdx.x * RS_HYP_BLOCK + threadIdx.x;
  if (h >= H) return;
  const size_t o0 = ((size_t)p * H + h) * 9, o1 = ((size_t)(gridDim.y + p) * H + h) * 9;
  const int n = ntot[p];
  bool good = n >= HomogModel::MIN;  // (below 4 the rejection loop of rs_sample would not end)
  double Hf[9], Hb[9];
  if (good) {
    const double *nm = norm + TV_NORM * (size_t)p;
    long long idx[4];
    rs_sample(seed, pairs[2 * p], pairs[2 * p + 1], h, n, idx);
    double pk[4][2], pl[4][2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double4 z = comp[(size_t)p * stride + idx[c]];
      pk[c][0] = nm[2] * (z.x - nm[0]); pk[c][1] = nm[2] * (z.y - nm[1]);
      pl[c][0] = nm[5] * (z.z - nm[3]); pl[c][1] = nm[5] * (z.w - nm[4]);
    }
    double Bk[9], Bl[9], hf[9], hb[9];
    const bool gk = hg_basis(pk, Bk), gl = hg_basis(pl, Bl);
    good = gk && gl;
    hg_map(Bl, Bk, hf);
    hg_map(Bk, Bl, hb);
    hg_denormalise(nm, nm + 3, hf, Hf);
    hg_denormalise(nm + 3, nm, hb, Hb);
#pragma unroll
    for (int e = 0; e < 9; ++e) good = good && isfinite(Hf[e]) && isfinite(Hb[e]);
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    hyp[o0 + e] = good ? Hf[e] : NAN;
    hyp[o1 + e] = good ? Hb[e] : NAN;
  }
  hyp_count[(size_t)p * H + h] = good ? 0 : -1;
}

// robust_pairs' model-specific steps for the homography (FundFit's counterpart)
struct HomogFit {
  using Model = HomogModel;
  static constexpr int MOMENTS = 4;
  static constexpr size_t HYP_BYTES = RS_HYP_BYTES;  // 72 H, 72 H^-1, 4 count, rounded up: what F^ and F take
  static constexpr const char *NAME = "H";
  static int prepare() { return MVBA_OK; }
  static void hypotheses(int cnt, long long stride, int H, unsigned long long seed, const int *pairs, const int *ntot, const double4 *comp,
                         const double *norm, double *hyp, int *hyp_count) {
    hipLaunchKernelGGL(k_homog_hyp, dim3((H + RS_HYP_BLOCK - 1) / RS_HYP_BLOCK, cnt), dim3(RS_HYP_BLOCK), 0, 0, stride, H, seed, pairs, ntot, comp,
                       norm, hyp, hyp_count);
  }
  // the best hypothesis is taken as the sample gives it, in the form the call returns
  static int finish(const double *Hbest, const double *, const double *, double *Hout) {
    std::copy(Hbest, Hbest + 9, Hout);
    return hg_unit(Hout) ? 0 : 2;
  }
  static int solve(const double *S45, const double *nm, double *Hout, double *ratio) { return homography_solve_pair(S45, nm, Hout, ratio); }
  static void mask_parts(const double *Hm, const double *nm, double *m0, double *m1) { hg_mask_parts(Hm, nm, m0, m1); }
};

}  // namespace

extern "C" {

int mvba_homography_sample(uint64_t seed, int32_t k, int32_t l, int32_t h, int64_t n, int64_t *idx4) {
  return sample_entry<HomogModel::MIN>(seed, "klh", k, l, h, n, idx4, "idx4", 6);
}

int mvba_homography_robust(int64_t n_points, int32_t n_images, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int64_t n_obs,
                           const int32_t *pairs, int32_t n_pairs, double threshold, int32_t n_hypotheses, uint64_t seed, int32_t n_refit,
                           double *H, double *quality, int64_t *n_shared, int64_t *n_inliers, int32_t *best, uint8_t *inlier,
                           int32_t *hyp_count, int32_t *status, double *timings_ms, int32_t device) {
  return robust_pairs<HomogFit>(n_points, n_images, pt_ptr, cam_idx, xy, n_obs, pairs, n_pairs, threshold, n_hypotheses, seed, n_refit, H, quality,
                                n_shared, n_inliers, best, inlier, hyp_count, status, timings_ms, device);
}

}  // extern "C"
