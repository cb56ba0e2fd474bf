// Robust triangulation (mvba_triangulate_robust, mvba_triangulate_sample): per-point two-view RANSAC -- kernels and host code,
// gfx950.
//
// Included by mvba.hip after mvba_resect_ransac.h: uses its rr_inlier, mvba_ransac.h's rs_sample, mvba_ransac_host.h's argument checks, mvba_init.h's
// init_camera_matrix, InitObsMasked and init_triangulate_point, mvba_start.h's checks, upload_list, InitClock, EvLaps and
// INIT_REL_PIVOT, and mvba.hip's DevBufs, fail and MVBA_HIP.  Nothing here runs on the LM path.  
//
// k_tri_score: a GROUP OF 16 LANES PER POINT, four points per wave.  A hypothesis is two of the point's observations; its
// model is the midpoint of their two viewing rays in closed form (two adjugates, no eigen-problem).  The group's lanes take
// the hypotheses h = lane, lane + 16, ...; a lane scores each of its own against all of the point's observations -- every
// lane of the group reads the same observation at the same step, so the loads of a group are one address --, keeps its
// running (count, h) in registers, and the group's best is an integer max of (count, -h) over four xor-shuffles of width 16.
// The best hypothesis's inlier set goes straight into the caller's byte per observation, lanes strided over the
// observations: there is no mask in registers or LDS, hence no degree limit.  k_tri_refit: ONE THREAD PER POINT, as
// k_triangulate: init_triangulate_point under that byte mask, the mask rewritten in place when a refit is kept.  The camera
// matrices sit in LDS in both, as in k_triangulate.  Counts are integers, every floating-point sum runs in ascending
// observation order inside one thread: no atomics of any kind, two calls return the same bits.

namespace {

constexpr int TR_GROUP = 16;      // lanes per point of k_tri_score
constexpr int TR_MAX_HYP = 4096;  // n_hypotheses

// The observation numbers i < j (below deg) of hypothesis h of point a; false where the table has no entry h.  All pairs in
// lexicographic order if they fit into H hypotheses, otherwise the first two draws of rs_sample(seed, a, a, h, deg), sorted.
__host__ __device__ __forceinline__ bool tri_pair(unsigned long long seed, int a, int h, int deg, int H, int &i, int &j) {
  const long long n_pairs = (long long)deg * (deg - 1) / 2;
  if (n_pairs <= H) {
    if (h >= n_pairs) return false;
    int r = h;
    i = 0;
    while (r >= deg - 1 - i) {
      r -= deg - 1 - i;
      ++i;
    }
    j = i + 1 + r;
    return true;
  }
  long long idx[2];
  rs_sample(seed, a, a, h, deg, idx);
  i = (int)(idx[0] < idx[1] ? idx[0] : idx[1]);
  j = (int)(idx[0] < idx[1] ? idx[1] : idx[0]);
  return true;
}

// d = M^-1 (x, y, 1) scaled to unit length, M = P[:, :3] inverted by its adjugate: the direction of the observation's viewing ray
__host__ __device__ __forceinline__ void tri_ray(const double *P, double2 z, double (&d)[3]) {
  const double a00 = P[5] * P[10] - P[6] * P[9], a01 = P[2] * P[9] - P[1] * P[10], a02 = P[1] * P[6] - P[2] * P[5];
  const double a10 = P[6] * P[8] - P[4] * P[10], a11 = P[0] * P[10] - P[2] * P[8], a12 = P[2] * P[4] - P[0] * P[6];
  const double a20 = P[4] * P[9] - P[5] * P[8], a21 = P[1] * P[8] - P[0] * P[9], a22 = P[0] * P[5] - P[1] * P[4];
  const double det = P[0] * a00 + P[1] * a10 + P[2] * a20;
  const double v0 = (a00 * z.x + a01 * z.y + a02) / det, v1 = (a10 * z.x + a11 * z.y + a12) / det, v2 = (a20 * z.x + a21 * z.y + a22) / det;
  const double n = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  d[0] = v0 / n; d[1] = v1 / n; d[2] = v2 / n;
}

// X = the midpoint of the common perpendicular of the rays c1 + s d1 and c2 + u d2; false if they are parallel to the
// relative pivot (1 - (d1 . d2)^2 <= 1e-12) or X is not finite
__host__ __device__ __forceinline__ bool tri_midpoint(const double *P1, const double *c1, double2 z1, const double *P2, const double *c2,
                                                      double2 z2, double (&X)[3]) {
  double d1[3], d2[3];
  tri_ray(P1, z1, d1);
  tri_ray(P2, z2, d2);
  const double b[3] = {c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]};
  const double al = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2], den = 1.0 - al * al;
  if (!(den > INIT_REL_PIVOT)) return false;  // (NaN too)
  const double b1 = b[0] * d1[0] + b[1] * d1[1] + b[2] * d1[2], b2 = b[0] * d2[0] + b[1] * d2[1] + b[2] * d2[2];
  const double s = (b1 - al * b2) / den, u = (al * b1 - b2) / den;
#pragma unroll
  for (int e = 0; e < 3; ++e) X[e] = 0.5 * (c1[e] + s * d1[e] + c2[e] + u * d2[e]);
  return init_finite(X[0]) && init_finite(X[1]) && init_finite(X[2]);
}

// hypothesis h of point a -> its midpoint; false if the table has no such entry or the hypothesis is degenerate
__device__ __forceinline__ bool tri_hypothesis(const InitObs &ob, const double *sP, const double *t, unsigned long long seed, int a, int h,
                                               int H, double (&X)[3]) {
  int i, j;
  if (!tri_pair(seed, a, h, ob.deg, H, i, j)) return false;
  const int k1 = ob.camera(i), k2 = ob.camera(j);
  return tri_midpoint(sP + 12 * k1, t + 3 * (size_t)k1, ob.xy[ob.o0 + i], sP + 12 * k2, t + 3 * (size_t)k2, ob.xy[ob.o0 + j], X);
}

// the number of the point's observations in front of their camera and within the threshold of X
__device__ __forceinline__ int tri_count(const InitObs &ob, const double *sP, const double (&X)[3], double thr2) {
  int c = 0;
  for (int i = 0; i < ob.deg; ++i) {
    double d2;
    c += rr_inlier(sP + 12 * ob.camera(i), X, ob.xy[ob.o0 + i], thr2, d2) ? 1 : 0;
  }
  return c;
}

__device__ __forceinline__ InitObs tri_obs(long long a, int m, const long long *pt_ptr, const int *cam_idx, const double2 *xy) {
  InitObs ob;
  ob.cam = pt_ptr ? cam_idx : nullptr;
  ob.xy = xy;
  ob.o0 = pt_ptr ? pt_ptr[a] : a * m;
  ob.deg = pt_ptr ? (int)(pt_ptr[a + 1] - pt_ptr[a]) : m;
  return ob;
}

// Hypotheses and scores.  Per point: status, best (-1 where no hypothesis is valid), n_inliers (0 where status != 0), X = the
// best midpoint (NaN where status != 0), the best hypothesis's inlier bytes (0 where status != 0), and, if asked for, the
// count table hyp_count [npts][H] (-1: no such hypothesis, or degenerate).
__global__ __launch_bounds__(256) void k_tri_score(long long npts, int m, const double *__restrict__ K, const double *__restrict__ R,
                                                   const double *__restrict__ t, const long long *__restrict__ pt_ptr,
                                                   const int *__restrict__ cam_idx, const double2 *__restrict__ xy, double thr2, int H,
                                                   unsigned long long seed, double *__restrict__ X, int *__restrict__ status,
                                                   int *__restrict__ n_inliers, int *__restrict__ best, unsigned char *__restrict__ inlier,
                                                   int *__restrict__ hyp_count) {
  extern __shared__ double sP[];  // [m][12]
  for (int k = threadIdx.x; k < m; k += blockDim.x) init_camera_matrix(K + 9 * (size_t)k, R + 9 * (size_t)k, t + 3 * (size_t)k, sP + 12 * k);
  __syncthreads();
  constexpr int PER_BLOCK = 256 / TR_GROUP;
  const int lane = threadIdx.x % TR_GROUP;
  const long long stride = (long long)gridDim.x * PER_BLOCK;
  // (a group's 16 lanes share a, so they leave this loop together: the shuffles below never read a lane that is gone)
  for (long long a = (long long)blockIdx.x * PER_BLOCK + threadIdx.x / TR_GROUP; a < npts; a += stride) {
    const InitObs ob = tri_obs(a, m, pt_ptr, cam_idx, xy);
    int bc = -1, bh = -1;
    for (int h = lane; h < H; h += TR_GROUP) {
      int cnt = -1;
      double Xh[3];
      if (ob.deg >= 2 && tri_hypothesis(ob, sP, t, seed, (int)a, h, H, Xh)) cnt = tri_count(ob, sP, Xh, thr2);
      if (hyp_count) hyp_count[(size_t)a * H + h] = cnt;
      if (cnt > bc) { bc = cnt; bh = h; }  // (h ascends: the lowest h of the lane's largest count)
    }
#pragma unroll
    for (int off = TR_GROUP / 2; off > 0; off >>= 1) {
      const int oc = __shfl_xor(bc, off, TR_GROUP), oh = __shfl_xor(bh, off, TR_GROUP);
      if (oc > bc || (oc == bc && oh < bh)) { bc = oc; bh = oh; }  // (bc = -1 goes with bh = -1 in every lane)
    }
    const int st = ob.deg < 2 ? 1 : (bc < 0 ? 2 : (bc < min(ob.deg, 3) ? 4 : 0));
    // every lane works the best midpoint out again -- the same arithmetic, the same bits -- and masks its share of the observations
    double Xb[3] = {NAN, NAN, NAN};
    if (st == 0) tri_hypothesis(ob, sP, t, seed, (int)a, bh, H, Xb);
    for (int i = lane; i < ob.deg; i += TR_GROUP) {
      double d2;
      inlier[ob.o0 + i] = (st == 0 && rr_inlier(sP + 12 * ob.camera(i), Xb, ob.xy[ob.o0 + i], thr2, d2)) ? 1 : 0;
    }
    if (lane == 0) {
      X[3 * a] = Xb[0]; X[3 * a + 1] = Xb[1]; X[3 * a + 2] = Xb[2];
      status[a] = st;
      n_inliers[a] = st == 0 ? bc : 0;
      best[a] = bh;
    }
  }
}

// Refits and quality, one thread per point of status 0: mvba_triangulate's fit on the current inliers alone, n_refit times at
// most.  The first is kept if it has min(deg, 3) inliers of its own, a later one while its set does not shrink; a fit whose
// status is not 0 ends the loop.  A kept fit's inlier set replaces the bytes in place (counted first, written once it is
// kept).  quality: mvba_triangulate's three figures over the final inliers at the final X.
__global__ __launch_bounds__(256) void k_tri_refit(long long npts, int m, const double *__restrict__ K, const double *__restrict__ R,
                                                   const double *__restrict__ t, const long long *__restrict__ pt_ptr,
                                                   const int *__restrict__ cam_idx, const double2 *__restrict__ xy, double thr2, int n_refine,
                                                   int n_refit, double *__restrict__ X, double *__restrict__ quality,
                                                   const int *__restrict__ status, int *__restrict__ n_inliers, unsigned char *inlier) {
  extern __shared__ double sP[];  // [m][12]
  for (int k = threadIdx.x; k < m; k += blockDim.x) init_camera_matrix(K + 9 * (size_t)k, R + 9 * (size_t)k, t + 3 * (size_t)k, sP + 12 * k);
  __syncthreads();
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x; a < npts; a += stride) {
    double q[3] = {NAN, NAN, NAN};
    if (status[a] == 0) {
      InitObsMasked ob;
      static_cast<InitObs &>(ob) = tri_obs(a, m, pt_ptr, cam_idx, xy);
      ob.mask = inlier;
      ob.n_used = n_inliers[a];
      double Xc[3] = {X[3 * a], X[3 * a + 1], X[3 * a + 2]};
      for (int r = 0; r < n_refit; ++r) {
        double Xr[3], qr[3];
        if (init_triangulate_point(ob, sP, R, t, n_refine, Xr, false, qr)) break;
        const int c = tri_count(ob, sP, Xr, thr2);
        if (c < (r == 0 ? min(ob.deg, 3) : ob.n_used)) break;
        for (int i = 0; i < ob.deg; ++i) {
          double d2;
          inlier[ob.o0 + i] = rr_inlier(sP + 12 * ob.camera(i), Xr, ob.xy[ob.o0 + i], thr2, d2) ? 1 : 0;
        }
        ob.n_used = c;
        Xc[0] = Xr[0]; Xc[1] = Xr[1]; Xc[2] = Xr[2];
      }
      double E = 0.0, dmin = HUGE_VAL, amax = 0.0;
      for (int i = 0; i < ob.deg; ++i) {
        if (!ob.use(i)) continue;
        const int k = ob.camera(i);
        double d2;
        rr_inlier(sP + 12 * k, Xc, ob.xy[ob.o0 + i], thr2, d2);
        E += d2;
        const double *Rk = R + 9 * (size_t)k, *tk = t + 3 * (size_t)k;
        const double a0 = Xc[0] - tk[0], a1 = Xc[1] - tk[1], a2 = Xc[2] - tk[2];
        dmin = fmin(dmin, Rk[2] * a0 + Rk[5] * a1 + Rk[8] * a2);
        for (int j = i + 1; j < ob.deg; ++j) {
          if (!ob.use(j)) continue;
          const double *tl = t + 3 * (size_t)ob.camera(j);
          const double b0 = Xc[0] - tl[0], b1 = Xc[1] - tl[1], b2 = Xc[2] - tl[2];
          const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
          amax = fmax(amax, atan2(sqrt(c0 * c0 + c1 * c1 + c2 * c2), a0 * b0 + a1 * b1 + a2 * b2));
        }
      }
      q[0] = sqrt(E / ob.n_used);
      q[1] = dmin;
      q[2] = amax;
      X[3 * a] = Xc[0]; X[3 * a + 1] = Xc[1]; X[3 * a + 2] = Xc[2];
      n_inliers[a] = ob.n_used;
    }
    quality[3 * a] = q[0]; quality[3 * a + 1] = q[1]; quality[3 * a + 2] = q[2];
  }
}

}  // namespace

extern "C" {

int mvba_triangulate_sample(uint64_t seed, int32_t point, int32_t h, int64_t deg, int32_t n_hypotheses, int64_t *idx2) {
  if (!idx2) return fail(MVBA_ERR_BADARG, "null argument: idx2 (argument 6)");
  if (deg < 2 || deg >= (1LL << 31)) return fail(MVBA_ERR_BADARG, "deg = " + std::to_string(deg) + " must be in 2 .. 2^31 - 1");
  if (n_hypotheses < 1 || n_hypotheses > TR_MAX_HYP)
    return fail(MVBA_ERR_BADARG, "n_hypotheses = " + std::to_string(n_hypotheses) + " must be in 1 .. " + std::to_string(TR_MAX_HYP));
  if (point < 0 || h < 0 || h >= n_hypotheses)
    return fail(MVBA_ERR_BADARG, "point = " + std::to_string(point) + ", h = " + std::to_string(h) + ": must be >= 0, and h < n_hypotheses = " +
                                     std::to_string(n_hypotheses));
  int i = -1, j = -1;
  if (!tri_pair(seed, point, h, (int)deg, n_hypotheses, i, j)) i = j = -1;
  idx2[0] = i;
  idx2[1] = j;
  return MVBA_OK;
}

int mvba_triangulate_robust(const double *K, const double *R, const double *t, int32_t n_images, int64_t n_points, const int64_t *pt_ptr,
                            const int32_t *cam_idx, const double *xy, int64_t n_obs, double threshold, int32_t n_hypotheses, uint64_t seed,
                            int32_t n_refine, int32_t n_refit, double *X, double *quality, int32_t *status, int32_t *n_inliers, int32_t *best,
                            uint8_t *inlier, int32_t *hyp_count, double *timings_ms, int32_t device) {
  if (!K || !R || !t || !xy || !X)
    return fail(MVBA_ERR_BADARG, std::string("null argument: ") + (!K ? "K" : (!R ? "R" : (!t ? "t" : (!xy ? "xy" : "X")))) + " (argument " +
                                     std::to_string(!K ? 1 : (!R ? 2 : (!t ? 3 : (!xy ? 8 : 15)))) + ")");
  int rc;
  if ((rc = rs_check_search(threshold, n_hypotheses, TR_MAX_HYP))) return rc;
  if (n_refine < 0) return fail(MVBA_ERR_BADARG, "n_refine = " + std::to_string(n_refine) + " must be >= 0");
  if ((rc = rs_check_refit(n_refit)) || (rc = init_check_list(n_points, n_images, pt_ptr, cam_idx, n_obs)) || (rc = init_check_cameras(n_images))) return rc;
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = timings_ms[3] = 0.0;
  if (n_points == 0) return MVBA_OK;
  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  const int H = n_hypotheses, m = n_images;
  InitClock clk;
  DevBufs tmp;  // (freed on every return)
  double *dK = nullptr, *dR = nullptr, *dt = nullptr, *dX = nullptr, *dq = nullptr;
  double2 *dxy = nullptr;
  long long *dptr = nullptr;
  int *dcam = nullptr, *dst = nullptr, *dni = nullptr, *dbest = nullptr, *dhc = nullptr;
  unsigned char *dinl = nullptr;
  if ((rc = tmp.alloc(&dK, 9 * (size_t)m)) || (rc = tmp.alloc(&dR, 9 * (size_t)m)) || (rc = tmp.alloc(&dt, 3 * (size_t)m)) ||
      (rc = tmp.alloc(&dX, 3 * (size_t)n_points)) || (rc = tmp.alloc(&dq, 3 * (size_t)n_points)) || (rc = tmp.alloc(&dst, (size_t)n_points)) ||
      (rc = tmp.alloc(&dni, (size_t)n_points)) || (rc = tmp.alloc(&dbest, (size_t)n_points)) ||
      (rc = tmp.alloc(&dinl, (size_t)std::max<int64_t>(n_obs, 1))))
    return rc;
  if (hyp_count && (rc = tmp.alloc(&dhc, (size_t)n_points * H))) return rc;
  MVBA_HIP(hipMemcpy(dK, K, sizeof(double) * 9 * m, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dR, R, sizeof(double) * 9 * m, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dt, t, sizeof(double) * 3 * m, hipMemcpyHostToDevice));
  if ((rc = upload_list(tmp, n_points, n_obs, pt_ptr, cam_idx, xy, &dptr, &dcam, &dxy))) return rc;
  const int lds = (int)(sizeof(double) * 12 * m);
  MVBA_HIP(hipFuncSetAttribute((const void *)k_tri_score, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  MVBA_HIP(hipFuncSetAttribute((const void *)k_tri_refit, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  EvLaps ev;
  if ((rc = ev.create(3))) return rc;
  if (timings_ms) timings_ms[0] = clk.lap();

  // both grids stop at 2048 workgroups and stride from there, as k_triangulate's does
  const int g_score = (int)std::max<long long>(1, std::min<long long>(2048, (n_points + 256 / TR_GROUP - 1) / (256 / TR_GROUP)));
  const int g_refit = (int)std::max<long long>(1, std::min<long long>(2048, (n_points + 255) / 256));
  const double thr2 = threshold * threshold;
  ev.mark();
  hipLaunchKernelGGL(k_tri_score, dim3(g_score), dim3(256), lds, 0, (long long)n_points, m, dK, dR, dt, dptr, dcam, dxy, thr2, H,
                     (unsigned long long)seed, dX, dst, dni, dbest, dinl, dhc);
  ev.mark();
  hipLaunchKernelGGL(k_tri_refit, dim3(g_refit), dim3(256), lds, 0, (long long)n_points, m, dK, dR, dt, dptr, dcam, dxy, thr2, n_refine, n_refit,
                     dX, dq, dst, dni, dinl);
  ev.mark();
  MVBA_HIP(hipGetLastError());
  MVBA_HIP(hipStreamSynchronize(0));
  if (timings_ms) {
    timings_ms[1] = ev.ms(0, 1);
    timings_ms[2] = ev.ms(1, 2);
  }
  clk.lap();  // (slot 3 is the download alone, not the rest of the wall time)
  MVBA_HIP(hipMemcpy(X, dX, sizeof(double) * 3 * n_points, hipMemcpyDeviceToHost));
  if (quality) MVBA_HIP(hipMemcpy(quality, dq, sizeof(double) * 3 * n_points, hipMemcpyDeviceToHost));
  if (status) MVBA_HIP(hipMemcpy(status, dst, sizeof(int) * n_points, hipMemcpyDeviceToHost));
  if (n_inliers) MVBA_HIP(hipMemcpy(n_inliers, dni, sizeof(int) * n_points, hipMemcpyDeviceToHost));
  if (best) MVBA_HIP(hipMemcpy(best, dbest, sizeof(int) * n_points, hipMemcpyDeviceToHost));
  if (inlier && n_obs) MVBA_HIP(hipMemcpy(inlier, dinl, (size_t)n_obs, hipMemcpyDeviceToHost));
  if (hyp_count) MVBA_HIP(hipMemcpy(hyp_count, dhc, sizeof(int) * (size_t)n_points * H, hipMemcpyDeviceToHost));
  if (timings_ms) timings_ms[3] = clk.lap();
  return MVBA_OK;
}

}  // extern "C"
