// Calibrated robust resection (mvba_pose_robust, mvba_pose_refine, mvba_pose_sample): P3P RANSAC for camera poses with known
// intrinsics and a pose-only Gauss-Newton refit against fixed points -- kernels and host code, gfx950.
//
// Included by mvba.hip after mvba_resect_ransac.h: uses its robust_cameras (the tile loop, with rr_inlier, k_resect_score,
// k_resect_mask and k_resect_scatter as they are: a hypothesis is scored as the 12-double matrix K [R^T | -R^T t]) and
// k_resect_gather, mvba_ransac.h's rs_sample, sample_entry and RS_HYP_BLOCK, mvba_ransac_host.h's argument checks,
// check_camera_list, rs_stop, rs_current and state bits, mvba_init.h's resect_build_list, CamWork and k_resect_combine, mvba_start.h's chunk_sum,
// init_check_list, InitClock and INIT_REL_PIVOT, and mvba.hip's DevBufs, fail and MVBA_HIP.  Nothing here runs on the LM path.
// 
//
// The usable observations are sorted camera-major as for mvba_resect_robust; the listed cameras get their own list of
// 256-observation chunks.  k_pose_hyp: one THREAD per hypothesis, registers only -- no LDS, no scratch: four observations,
// their bearings through K^-1 (the adjugate), the quartic of the three-point pose problem in v = s2 / s0, its real roots by
// Ferrari's factorisation into two quadratics (a positive root of the resolvent cubic by Newton's iteration inside a bracket,
// bisection where it would leave it: a fixed trip count), each polished on the quartic and then by three Newton steps on the three
// cosine-law equations, the pose of each by two Gram-Schmidt frames, the fourth observation picks one.  Scoring, the best
// hypothesis and the masks are mvba_resect_robust's.  A refit is n_refine Gauss-Newton steps on the reprojection error over the
// inlier mask: k_pose_fit sums the 29 values of a pass by chunk_sum, k_resect_combine adds a camera's chunks in ascending
// order, k_pose_step (one thread per camera) holds the accept rule, the 6 x 6 Cholesky and the pose update -- the host sees a
// refit once, when it ends.  No floating-point atomics: two calls return the same bits.

namespace {

constexpr int PR_MIN_OBS = 4;          // three observations for the pose, a fourth to choose among its solutions
constexpr int PR_MIN_REFINE_OBS = 3;   // mvba_pose_refine: six unknowns need three observations
constexpr size_t PR_HYP_BYTES = 196;   // device bytes per hypothesis of a camera of a tile: 96 P, 96 pose, 4 count
constexpr int PR_MAX_REFINE = 16;      // n_refine of mvba_pose_robust
constexpr int PR_MAX_STEPS = 64;       // n_steps of mvba_pose_refine
constexpr int PR_NV = 29;              // values of a pass: 21 of J^T J, 6 of J^T e, the cost, the count
constexpr int PR_ROOT_ITERS = 50;      // steps for a root of the resolvent: Newton inside a bracket, bisection where it leaves it
// the Gauss-Newton record of a camera: cost of the previous pose, of the first, of the current one, the observation count, the
// smallest relative pivot of the last solve, steps taken, the step whose normal matrix failed the pivot rule (-1: none)
enum { PG_PREV = 0, PG_COST0, PG_COST, PG_COUNT, PG_PIVOT, PG_STEPS, PG_FAIL, PG_SIZE = 8 };

// d = K^-1 (x, y, 1) scaled to unit length, K (3 x 3 row-major) inverted by its adjugate (tri_ray's form, for K alone)
__host__ __device__ __forceinline__ void pose_bearing(const double *K, double2 z, double (&d)[3]) {
  const double a00 = K[4] * K[8] - K[5] * K[7], a01 = K[2] * K[7] - K[1] * K[8], a02 = K[1] * K[5] - K[2] * K[4];
  const double a10 = K[5] * K[6] - K[3] * K[8], a11 = K[0] * K[8] - K[2] * K[6], a12 = K[2] * K[3] - K[0] * K[5];
  const double a20 = K[3] * K[7] - K[4] * K[6], a21 = K[1] * K[6] - K[0] * K[7], a22 = K[0] * K[4] - K[1] * K[3];
  const double det = K[0] * a00 + K[1] * a10 + K[2] * a20;
  const double v0 = (a00 * z.x + a01 * z.y + a02) / det, v1 = (a10 * z.x + a11 * z.y + a12) / det, v2 = (a20 * z.x + a21 * z.y + a22) / det;
  const double n = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  d[0] = v0 / n; d[1] = v1 / n; d[2] = v2 / n;
}

// P (3 x 4 row-major) = K [R^T | -R^T t]; R row-major with the camera axes in its columns, t the centre
__host__ __device__ __forceinline__ void pose_matrix(const double *K, const double *R, const double *t, double *P) {
  double M[12];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    M[4 * i] = R[i]; M[4 * i + 1] = R[3 + i]; M[4 * i + 2] = R[6 + i];
    M[4 * i + 3] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) P[4 * r + c] = K[3 * r] * M[c] + K[3 * r + 1] * M[4 + c] + K[3 * r + 2] * M[8 + c];
}

// the orthonormal frame of the triangle (A0, A1, A2): e1 along 1 - 0, e2 along 2 - 0 with its e1 part removed, e3 = e1 x e2;
// false if the remainder's squared length is <= 1e-12 x that of the edge 2 - 0
__host__ __device__ __forceinline__ bool pose_frame(const double *A0, const double *A1, const double *A2, double (&e1)[3], double (&e2)[3],
                                                    double (&e3)[3]) {
  double w[3];
  double n1 = 0.0, n2 = 0.0, dot = 0.0, nr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) { e1[i] = A1[i] - A0[i]; w[i] = A2[i] - A0[i]; n1 += e1[i] * e1[i]; n2 += w[i] * w[i]; }
  n1 = sqrt(n1);
#pragma unroll
  for (int i = 0; i < 3; ++i) { e1[i] /= n1; dot += e1[i] * w[i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) { e2[i] = w[i] - dot * e1[i]; nr += e2[i] * e2[i]; }
  const double ln = sqrt(nr);
#pragma unroll
  for (int i = 0; i < 3; ++i) e2[i] /= ln;
  e3[0] = e1[1] * e2[2] - e1[2] * e2[1];
  e3[1] = e1[2] * e2[0] - e1[0] * e2[2];
  e3[2] = e1[0] * e2[1] - e1[1] * e2[0];
  return nr > INIT_REL_PIVOT * n2;
}

// The pose of a camera with intrinsics K from three points and their images, the one of its (at most four) solutions that
// images a fourth point best: R [9], t [3] and P = K [R^T | -R^T t].  false: no solution in front of which Xs[3] lies, a
// degenerate triangle, or something not finite.  Registers only: every array index is a compile-time constant once unrolled.
__host__ __device__ __forceinline__ bool pose_p3p(const double *K, const double (&Xs)[4][3], const double2 (&zs)[4], double *R, double *t,
                                                  double *P) {
  double d0[3], d1[3], d2[3];
  pose_bearing(K, zs[0], d0);
  pose_bearing(K, zs[1], d1);
  pose_bearing(K, zs[2], d2);
  double fx1[3], fx2[3], fx3[3];
  const bool frame_ok = pose_frame(Xs[0], Xs[1], Xs[2], fx1, fx2, fx3);
  double a2 = 0.0, b2 = 0.0, c2 = 0.0, ca = 0.0, cb = 0.0, cg = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double e12 = Xs[1][i] - Xs[2][i], e02 = Xs[0][i] - Xs[2][i], e01 = Xs[0][i] - Xs[1][i];
    a2 += e12 * e12; b2 += e02 * e02; c2 += e01 * e01;
    ca += d1[i] * d2[i]; cb += d0[i] * d2[i]; cg += d0[i] * d1[i];
  }
  // u = N(v) / D(v) with N = q W - v^2 + 1, D = 2 (cos gamma - v cos alpha), W = 1 + v^2 - 2 v cos beta; the third equation
  // times D^2: D^2 (1 - r W) + N^2 - 2 cos gamma N D = 0, r = c^2 / b^2
  const double q = (a2 - c2) / b2, r = c2 / b2;
  const double n2 = q - 1.0, n1 = -2.0 * q * cb, n0 = q + 1.0, dd1 = -2.0 * ca, dd0 = 2.0 * cg;
  const double e2 = dd1 * dd1, e1 = 2.0 * dd0 * dd1, e0 = dd0 * dd0, f2 = -r, f1 = 2.0 * r * cb, f0 = 1.0 - r;
  const double A4 = e2 * f2 + n2 * n2;
  const double A3 = e2 * f1 + e1 * f2 + 2.0 * n2 * n1 - 2.0 * cg * (n2 * dd1);
  const double A2 = e2 * f0 + e1 * f1 + e0 * f2 + 2.0 * n2 * n0 + n1 * n1 - 2.0 * cg * (n2 * dd0 + n1 * dd1);
  const double A1 = e1 * f0 + e0 * f1 + 2.0 * n1 * n0 - 2.0 * cg * (n1 * dd0 + n0 * dd1);
  const double A0 = e0 * f0 + n0 * n0 - 2.0 * cg * (n0 * dd0);
  // monic, depressed by v = y - B3 / 4: y^4 + p y^2 + g y + h
  const double B3 = A3 / A4, B2 = A2 / A4, B1 = A1 / A4, B0 = A0 / A4;
  const double p = B2 - 0.375 * B3 * B3, g = B1 - 0.5 * B3 * B2 + 0.125 * B3 * B3 * B3;
  const double h = B0 - 0.25 * B3 * B1 + 0.0625 * B3 * B3 * B2 - (3.0 / 256.0) * B3 * B3 * B3 * B3;
  // Ferrari: (y^2 + p / 2 + m)^2 = 2 m (y - g / (4 m))^2 for a root m > 0 of m^3 + p m^2 + (p^2 / 4 - h) m - g^2 / 8: the
  // cubic is <= 0 at 0 and > 0 at 1 + its largest coefficient magnitude; Newton where it stays inside the bracket
  const double k2 = p, k1 = 0.25 * p * p - h, k0 = -0.125 * g * g;
  double hi = 1.0 + fmax(fabs(k2), fmax(fabs(k1), fabs(k0))), lo = 0.0, m = hi;
  for (int it = 0; it < PR_ROOT_ITERS; ++it) {
    const double fv = ((m + k2) * m + k1) * m + k0, fd = (3.0 * m + 2.0 * k2) * m + k1;
    if (fv > 0.0) hi = m; else lo = m;
    const double mn = m - fv / fd;
    m = (mn > lo && mn < hi) ? mn : 0.5 * (lo + hi);
  }
  const double s = sqrt(2.0 * m), gs = g / (2.0 * s);
  const double q1 = 0.5 * p + m - gs, q2 = 0.5 * p + m + gs;  // y^2 + s y + q1 = 0, y^2 - s y + q2 = 0
  const double D1 = s * s - 4.0 * q1, D2 = s * s - 4.0 * q2;
  bool found = false;
  double best_d2 = HUGE_VAL, best_s0 = HUGE_VAL;
  for (int c = 0; c < 4; ++c) {
    const double disc = (c & 2) ? D2 : D1;
    const double root = sqrt(disc);
    const double y = 0.5 * (((c & 2) ? s : -s) + ((c & 1) ? root : -root));
    double v = y - 0.25 * B3;
#pragma unroll
    for (int it = 0; it < 2; ++it) {  // polish on the quartic itself
      const double fv = (((v + B3) * v + B2) * v + B1) * v + B0, fd = ((4.0 * v + 3.0 * B3) * v + 2.0 * B2) * v + B1;
      const double vn = v - fv / fd;
      v = isfinite(vn) ? vn : v;
    }
    const double W = 1.0 + v * v - 2.0 * v * cb;
    const double u = ((n2 * v + n1) * v + n0) / (dd1 * v + dd0);
    double s0 = sqrt(b2 / W), s1 = u * s0, s2 = v * s0;
    bool ok = frame_ok && disc >= 0.0 && s0 > 0.0 && s1 > 0.0 && s2 > 0.0;
    if (!ok) continue;
#pragma unroll
    for (int it = 0; it < 3; ++it) {  // Newton on the three equations: a 3 x 3 solve by the adjugate
      const double F1 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * ca - a2, F2 = s0 * s0 + s2 * s2 - 2.0 * s0 * s2 * cb - b2,
                   F3 = s0 * s0 + s1 * s1 - 2.0 * s0 * s1 * cg - c2;
      const double j01 = 2.0 * (s1 - s2 * ca), j02 = 2.0 * (s2 - s1 * ca), j10 = 2.0 * (s0 - s2 * cb), j12 = 2.0 * (s2 - s0 * cb),
                   j20 = 2.0 * (s0 - s1 * cg), j21 = 2.0 * (s1 - s0 * cg);
      // J = [[0, j01, j02], [j10, 0, j12], [j20, j21, 0]]
      const double det = j01 * j12 * j20 + j02 * j10 * j21;
      const double x0 = (-j12 * j21) * F1 + (j02 * j21) * F2 + (j01 * j12) * F3;
      const double x1 = (j12 * j20) * F1 + (-j02 * j20) * F2 + (j02 * j10) * F3;
      const double x2 = (j10 * j21) * F1 + (j01 * j20) * F2 + (-j01 * j10) * F3;
      s0 -= x0 / det; s1 -= x1 / det; s2 -= x2 / det;
    }
    ok = s0 > 0.0 && s1 > 0.0 && s2 > 0.0 && isfinite(s0) && isfinite(s1) && isfinite(s2);
    if (!ok) continue;
    double Y0[3], Y1[3], Y2[3], fy1[3], fy2[3], fy3[3], Rc[9], tc[3], Pc[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) { Y0[i] = s0 * d0[i]; Y1[i] = s1 * d1[i]; Y2[i] = s2 * d2[i]; }
    if (!pose_frame(Y0, Y1, Y2, fy1, fy2, fy3)) continue;
    // R_cw = F_Y F_X^T, R = R_cw^T: R[i][j] = sum_k fx_k[i] fy_k[j]; t = X0 - R Y0
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Rc[3 * i + j] = fx1[i] * fy1[j] + fx2[i] * fy2[j] + fx3[i] * fy3[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) tc[i] = Xs[0][i] - (Rc[3 * i] * Y0[0] + Rc[3 * i + 1] * Y0[1] + Rc[3 * i + 2] * Y0[2]);
    pose_matrix(K, Rc, tc, Pc);
    double dist;
    bool fin = rr_inlier(Pc, Xs[3], zs[3], HUGE_VAL, dist);  // in front, and a distance that is a number
#pragma unroll
    for (int e = 0; e < 12; ++e) fin = fin && isfinite(Pc[e]);
#pragma unroll
    for (int e = 0; e < 9; ++e) fin = fin && isfinite(Rc[e]);
    fin = fin && isfinite(tc[0]) && isfinite(tc[1]) && isfinite(tc[2]);
    if (fin && (dist < best_d2 || (dist == best_d2 && s0 < best_s0))) {
      found = true;
      best_d2 = dist;
      best_s0 = s0;
#pragma unroll
      for (int e = 0; e < 9; ++e) R[e] = Rc[e];
#pragma unroll
      for (int e = 0; e < 3; ++e) t[e] = tc[e];
#pragma unroll
      for (int e = 0; e < 12; ++e) P[e] = Pc[e];
    }
  }
  return found;
}

// One thread per hypothesis of camera cam0 + blockIdx.y of the list: the four indices, pose_p3p -> hypP [tile camera][H][12]
// and hypRt [tile camera][H][12] (R, then t); hyp_count = 0, or -1 (and NaN) if degenerate.
__global__ __launch_bounds__(RS_HYP_BLOCK) void k_pose_hyp(int cam0, int H, unsigned long long seed, const int *__restrict__ cams,
                                                           const long long *__restrict__ lc_start, const int *__restrict__ lc_n,
                                                           const int *__restrict__ cm_pt, const double2 *__restrict__ cm_xy,
                                                           const double *__restrict__ X, const double *__restrict__ Kc,
                                                           double *__restrict__ hypP, double *__restrict__ hypRt, int *__restrict__ hyp_count) {
  const int kl = blockIdx.y, k = cam0 + kl, h = blockIdx.x * RS_HYP_BLOCK + threadIdx.x;
  if (h >= H) return;
  const size_t oh = (size_t)kl * H + h;
  const int n = lc_n[k];
  bool good = n >= PR_MIN_OBS;  // (below 4 the rejection loop of rs_sample would not end)
  double P[12], Rt[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) P[e] = Rt[e] = NAN;
  if (good) {
    long long idx[4];
    rs_sample(seed, cams[k], cams[k], h, n, idx);
    double Xs[4][3], Kk[9];
    double2 zs[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long long o = lc_start[k] + idx[c];
      const double *Xp = X + 3 * (size_t)cm_pt[o];
      Xs[c][0] = Xp[0]; Xs[c][1] = Xp[1]; Xs[c][2] = Xp[2];
      zs[c] = cm_xy[o];
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) Kk[e] = Kc[9 * (size_t)k + e];
    good = pose_p3p(Kk, Xs, zs, Rt, Rt + 9, P);
  }
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    hypP[oh * 12 + e] = good ? P[e] : NAN;
    hypRt[oh * 12 + e] = good ? Rt[e] : NAN;
  }
  hyp_count[oh] = good ? 0 : -1;
}

// The 29 values of one observation at the pose (R, t) under K: e = pi(K R^T (X - t)) - xy, J = de / d(delta t, omega) with
// t <- t + delta t, R <- Rod(omega) R: with d = X - t and A = (d pi / d y) R^T, J = [-A | rows of A x d].
__device__ __forceinline__ void pose_pass(const double *K, const double *R, const double *t, const double *Xa, double2 z, double (&v)[PR_NV]) {
  const double d[3] = {Xa[0] - t[0], Xa[1] - t[1], Xa[2] - t[2]};
  double y[3], p[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = R[i] * d[0] + R[3 + i] * d[1] + R[6 + i] * d[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) p[r] = K[3 * r] * y[0] + K[3 * r + 1] * y[1] + K[3 * r + 2] * y[2];
  const double pi[2] = {p[0] / p[2], p[1] / p[2]};
  const double e[2] = {pi[0] - z.x, pi[1] - z.y};
  double J[2][6];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    double jy[3], a[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) jy[i] = (K[3 * r + i] - pi[r] * K[6 + i]) / p[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) a[j] = jy[0] * R[3 * j] + jy[1] * R[3 * j + 1] + jy[2] * R[3 * j + 2];
    J[r][0] = -a[0]; J[r][1] = -a[1]; J[r][2] = -a[2];
    J[r][3] = a[1] * d[2] - a[2] * d[1];
    J[r][4] = a[2] * d[0] - a[0] * d[2];
    J[r][5] = a[0] * d[1] - a[1] * d[0];
  }
  int n = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b, ++n) v[n] = J[0][a] * J[0][b] + J[1][a] * J[1][b];
#pragma unroll
  for (int a = 0; a < 6; ++a) v[21 + a] = J[0][a] * e[0] + J[1][a] * e[1];
  v[27] = e[0] * e[0] + e[1] * e[1];
  v[28] = 1.0;
}

// One pass of a refit: the 29 sums of each chunk over the observations whose byte in the camera's current mask is set, at
// the camera's current pose.  A camera that is not RS_ACTIVE, or whose iteration has ended (gflag, unless first), sums nothing.
__global__ __launch_bounds__(START_CHUNK) void k_pose_fit(int first, const int *__restrict__ ch_cam, const long long *__restrict__ ch_start,
                                                          const long long *__restrict__ ch_mask, const int *__restrict__ ch_cnt,
                                                          const int *__restrict__ cm_pt, const double2 *__restrict__ cm_xy,
                                                          const double *__restrict__ X, const int *__restrict__ state,
                                                          const unsigned char *__restrict__ inl0, const unsigned char *__restrict__ inl1,
                                                          const int *__restrict__ gflag, const double *__restrict__ Kc,
                                                          const double *__restrict__ pose, double *__restrict__ part) {
  __shared__ double s_w[START_CHUNK / 64][PR_NV];
  const int c = blockIdx.x, k = ch_cam[c], i = threadIdx.x, st = state[k];
  double v[PR_NV];
#pragma unroll
  for (int e = 0; e < PR_NV; ++e) v[e] = 0.0;
  if ((st & RS_ACTIVE) && (first || !gflag[k]) && i < ch_cnt[c] && rs_current(st, inl0, inl1)[ch_mask[c] + i]) {
    const long long o = ch_start[c] + i;
    double Kk[9], Rt[12];
#pragma unroll
    for (int e = 0; e < 9; ++e) Kk[e] = Kc[9 * (size_t)k + e];
#pragma unroll
    for (int e = 0; e < 12; ++e) Rt[e] = pose[12 * (size_t)k + e];
    pose_pass(Kk, Rt, Rt + 9, X + 3 * (size_t)cm_pt[o], cm_xy[o], v);
  }
  chunk_sum<PR_NV>(v, s_w, part + (size_t)c * PR_NV);
}

// Step j of n_steps of a refit, one thread per camera of the tile, after pass j's sums S [cnt][29].  j = 0 starts the record.
// The pose of pass j is kept if its cost does not exceed the previous one (mvba_triangulate's rule), otherwise the previous
// pose comes back and the camera's iteration ends; it also ends after n_steps, and where the normal matrix fails the pivot
// rule (PG_FAIL = j).  Otherwise delta = -(J^T J)^-1 J^T e by Cholesky, t <- t + delta t, R <- Rod(omega) R.
__global__ __launch_bounds__(256) void k_pose_step(int cnt, int j, int n_steps, const int *__restrict__ state, const double *__restrict__ S,
                                                   double *__restrict__ pose, double *__restrict__ prev, double *__restrict__ gn,
                                                   int *__restrict__ gflag) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt || !(state[k] & RS_ACTIVE)) return;
  const double *s = S + PR_NV * (size_t)k;
  double *rec = gn + PG_SIZE * (size_t)k, *ps = pose + 12 * (size_t)k, *pv = prev + 12 * (size_t)k;
  const double cost = s[27];
  if (j == 0) {
    bool fin = isfinite(cost);
    for (int e = 0; e < 12; ++e) fin = fin && isfinite(ps[e]);
    rec[PG_PREV] = rec[PG_COST0] = rec[PG_COST] = cost;
    rec[PG_COUNT] = s[28];
    rec[PG_PIVOT] = 0.0;
    rec[PG_STEPS] = 0.0;
    rec[PG_FAIL] = fin ? -1.0 : 0.0;
    gflag[k] = fin ? 0 : 1;
    if (!fin) return;
  } else {
    if (gflag[k]) return;
    if (!(cost <= rec[PG_PREV])) {
      for (int e = 0; e < 12; ++e) ps[e] = pv[e];
      gflag[k] = 1;
      return;
    }
    rec[PG_STEPS] += 1.0;
    rec[PG_COST] = cost;
  }
  if (j == n_steps) {
    gflag[k] = 1;
    return;
  }
  double Hm[6][6], gv[6];
  {
    int n = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b, ++n) Hm[a][b] = Hm[b][a] = s[n];
#pragma unroll
    for (int a = 0; a < 6; ++a) gv[a] = s[21 + a];
  }
  double dmax = Hm[0][0];
#pragma unroll
  for (int a = 1; a < 6; ++a) dmax = fmax(dmax, Hm[a][a]);
  // Cholesky in place (the lower triangle becomes L); a pivot is the diagonal entry before its square root
  bool good = true;
  double pmin = HUGE_VAL;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double piv = Hm[a][a];
#pragma unroll
    for (int c = 0; c < a; ++c) piv -= Hm[a][c] * Hm[a][c];
    good = good && piv > INIT_REL_PIVOT * dmax;
    pmin = fmin(pmin, piv / dmax);
    const double l = sqrt(piv);
    Hm[a][a] = l;
#pragma unroll
    for (int b = a + 1; b < 6; ++b) {
      double x = Hm[b][a];
#pragma unroll
      for (int c = 0; c < a; ++c) x -= Hm[b][c] * Hm[a][c];
      Hm[b][a] = x / l;
    }
  }
  if (!good) {  // (a NaN pivot fails the comparison too)
    rec[PG_FAIL] = (double)j;
    gflag[k] = 1;
    return;
  }
  rec[PG_PIVOT] = pmin;
  double x[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) {  // L w = -g
    double w = -gv[a];
#pragma unroll
    for (int c = 0; c < a; ++c) w -= Hm[a][c] * x[c];
    x[a] = w / Hm[a][a];
  }
#pragma unroll
  for (int a = 5; a >= 0; --a) {  // L^T delta = w
    double w = x[a];
#pragma unroll
    for (int c = a + 1; c < 6; ++c) w -= Hm[c][a] * x[c];
    x[a] = w / Hm[a][a];
  }
  double Rn[9];
  {  // Rod(omega) = cos I + sin [n]x + (1 - cos) n n^T, exactly I at omega = 0
    const double th = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
    double Q[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (th > 0.0) {
      const double n0 = x[3] / th, n1 = x[4] / th, n2 = x[5] / th, cs = cos(th), sn = sin(th), oc = 1.0 - cs;
      Q[0] = cs + oc * n0 * n0; Q[1] = oc * n0 * n1 - sn * n2; Q[2] = oc * n0 * n2 + sn * n1;
      Q[3] = oc * n1 * n0 + sn * n2; Q[4] = cs + oc * n1 * n1; Q[5] = oc * n1 * n2 - sn * n0;
      Q[6] = oc * n2 * n0 - sn * n1; Q[7] = oc * n2 * n1 + sn * n0; Q[8] = cs + oc * n2 * n2;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) Rn[3 * a + b] = Q[3 * a] * ps[b] + Q[3 * a + 1] * ps[3 + b] + Q[3 * a + 2] * ps[6 + b];
  }
  for (int e = 0; e < 12; ++e) pv[e] = ps[e];
  rec[PG_PREV] = cost;
  for (int e = 0; e < 9; ++e) ps[e] = Rn[e];
  for (int e = 0; e < 3; ++e) ps[9 + e] += x[e];
}

// P[camera] = K [R^T | -R^T t] of the current poses of the cnt cameras of a tile
__global__ __launch_bounds__(256) void k_pose_matrix(int cnt, const double *__restrict__ Kc, const double *__restrict__ pose, double *__restrict__ P) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  double Kk[9], Rt[12], Pk[12];
  for (int e = 0; e < 9; ++e) Kk[e] = Kc[9 * (size_t)k + e];
  for (int e = 0; e < 12; ++e) Rt[e] = pose[12 * (size_t)k + e];
  pose_matrix(Kk, Rt, Rt + 9, Pk);
  for (int e = 0; e < 12; ++e) P[12 * (size_t)k + e] = Pk[e];
}

// The Gauss-Newton passes 0 .. n_steps of the cnt cameras from list position c0 on, enqueued without a host round trip:
// per pass the sums of the tile's chunks, a camera's chunks combined in ascending order, the step.
void pose_iterate(const CamWork &w, int c0, int cnt, int n_steps, const int *dstate, const unsigned char *dinl0, const unsigned char *dinl1,
                  double *dpose, double *dprev, double *dgn, int *dgflag, double *dpart, double *dS) {
  const int ch0 = w.lc_ch[c0], tch = w.lc_ch[c0 + cnt] - ch0;
  for (int j = 0; j <= n_steps; ++j) {
    if (tch > 0)
      hipLaunchKernelGGL(k_pose_fit, dim3((unsigned)tch), dim3(START_CHUNK), 0, 0, j == 0 ? 1 : 0, w.dch_cam + ch0, w.dch_start + ch0, w.dch_mask + ch0,
                         w.dch_cnt + ch0, w.dpt, w.dxy, w.dX, dstate, dinl0, dinl1, dgflag, w.dK, dpose, dpart + PR_NV * (size_t)ch0);
    hipLaunchKernelGGL(k_resect_combine, dim3((cnt * PR_NV + 255) / 256), dim3(256), 0, 0, cnt, PR_NV, w.dlc_ch + c0, dpart, dS);
    hipLaunchKernelGGL(k_pose_step, dim3((cnt + 255) / 256), dim3(256), 0, 0, cnt, j, n_steps, dstate + c0, dS, dpose + 12 * (size_t)c0,
                       dprev + 12 * (size_t)c0, dgn + PG_SIZE * (size_t)c0, dgflag + c0);
  }
}

// The calibrated pose as a fit: nothing before the hypotheses, which also give (R, t); a refit is pose_iterate on the device.
struct PoseFit {
  static constexpr int MIN_OBS = PR_MIN_OBS, NV = PR_NV;
  static constexpr size_t HYP_BYTES = PR_HYP_BYTES;
  static constexpr long long FIRST_MIN = 0;  // (the first refit is held to the kept count as every later one)
  double *R, *t;  // [n_cameras][9], [n_cameras][3], out
  int n_refine;
  double *dhypRt = nullptr, *dpose = nullptr, *dprev = nullptr, *dgn = nullptr;
  int *dscore_n = nullptr, *dgflag = nullptr;
  std::vector<double> Rc, Rn, gn, pivot;

  int setup(DevBufs &tmp, const CamWork &w, int tile, int H) {
    const size_t nl = w.cams.size();
    int rc;
    if ((rc = tmp.alloc(&dpose, 12 * nl)) || (rc = tmp.alloc(&dprev, 12 * nl)) || (rc = tmp.alloc(&dgn, PG_SIZE * nl)) || (rc = tmp.alloc(&dgflag, nl)) ||
        (rc = tmp.alloc(&dscore_n, nl)) || (rc = tmp.alloc(&dhypRt, 12 * (size_t)tile * H)))
      return rc;
    // k_resect_score leaves a camera below ITS minimum alone: it is told 6 for every camera that has the 4 this one needs
    std::vector<int> score_n(nl);
    for (size_t c = 0; c < nl; ++c) score_n[c] = w.lc_n[c] >= PR_MIN_OBS ? std::max(w.lc_n[c], RR_MIN_OBS) : 0;
    MVBA_HIP(hipMemcpy(dscore_n, score_n.data(), sizeof(int) * nl, hipMemcpyHostToDevice));
    Rc.resize(12 * (size_t)tile); Rn.resize(12 * (size_t)tile); gn.resize(PG_SIZE * (size_t)tile); pivot.resize((size_t)tile);
    return MVBA_OK;
  }
  const int *score_n(const CamWork &) const { return dscore_n; }
  void hypotheses(const CamTile &c) {
    const CamWork &w = c.w;
    hipLaunchKernelGGL(k_pose_hyp, dim3((c.H + RS_HYP_BLOCK - 1) / RS_HYP_BLOCK, c.cnt), dim3(RS_HYP_BLOCK), 0, 0, c.c0, c.H, c.seed, w.dcams, w.dlc_start,
                       w.dlc_n, w.dpt, w.dxy, w.dX, w.dK, c.dhypP, dhypRt, c.dhc);
  }
  void picked(const CamTile &c, const int *dbest) {
    hipLaunchKernelGGL(k_resect_gather, dim3((c.cnt * 12 + 255) / 256), dim3(256), 0, 0, c.cnt, c.H, dbest, dhypRt, dpose + 12 * (size_t)c.c0);
  }
  int fetch(const CamTile &c, bool first) {
    MVBA_HIP(hipMemcpy((first ? Rc : Rn).data(), dpose + 12 * (size_t)c.c0, sizeof(double) * 12 * c.cnt, hipMemcpyDeviceToHost));
    if (first) std::fill(pivot.begin(), pivot.end(), 0.0);  // (no refit kept yet)
    return MVBA_OK;
  }
  // n_refine Gauss-Newton steps over the current inliers, all on the device
  int refit(const CamTile &c, int *tstate, int &n_active) {
    pose_iterate(c.w, c.c0, c.cnt, n_refine, c.dstate, c.dinl0, c.dinl1, dpose, dprev, dgn, dgflag, c.dpart, c.dS);
    hipLaunchKernelGGL(k_pose_matrix, c.gc, dim3(256), 0, 0, c.cnt, c.w.dK + 9 * (size_t)c.c0, dpose + 12 * (size_t)c.c0, c.dP + 12 * (size_t)c.c0);
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(gn.data(), dgn + PG_SIZE * (size_t)c.c0, sizeof(double) * PG_SIZE * c.cnt, hipMemcpyDeviceToHost));
    for (int p = 0; p < c.cnt; ++p)
      if ((tstate[p] & RS_ACTIVE) && gn[PG_SIZE * (size_t)p + PG_FAIL] >= 0.0) rs_stop(tstate[p], n_active);  // the pivot rule, or a pose that is not finite
    return MVBA_OK;
  }
  void keep(int p) {
    if (n_refine > 0) pivot[p] = gn[PG_SIZE * (size_t)p + PG_PIVOT];
    for (int j = 0; j < 12; ++j) Rc[12 * (size_t)p + j] = Rn[12 * (size_t)p + j];
  }
  double output(int p, size_t g) const {
    for (int j = 0; j < 9; ++j) R[9 * g + j] = Rc[12 * (size_t)p + j];
    for (int j = 0; j < 3; ++j) t[3 * g + j] = Rc[12 * (size_t)p + 9 + j];
    return pivot[p];
  }
};

}  // namespace

extern "C" {

int mvba_pose_sample(uint64_t seed, int32_t k, int32_t h, int64_t n, int64_t *idx4) {
  return sample_entry<PR_MIN_OBS>(seed, "kh", k, k, h, n, idx4, "idx4", 5);
}

int mvba_pose_robust(const double *X, int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int64_t n_obs,
                     int32_t n_images, const uint8_t *point_ok, const double *K, const int32_t *cameras, int32_t n_cameras, double threshold,
                     int32_t n_hypotheses, uint64_t seed, int32_t n_refine, int32_t n_refit, double *R, double *t, double *quality,
                     int64_t *n_usable, int64_t *n_inliers, int32_t *best, uint8_t *inlier, int32_t *hyp_count, int32_t *status,
                     double *timings_ms, int32_t device) {
  if (n_cameras < 0) return fail(MVBA_ERR_BADARG, "n_cameras = " + std::to_string(n_cameras) + " must be >= 0");
  if (!X || !xy || !K || (n_cameras > 0 && (!R || !t)))
    return fail(MVBA_ERR_BADARG, std::string("null argument: ") + (!X ? "X" : (!xy ? "xy" : (!K ? "K" : (!R ? "R" : "t")))) + " (argument " +
                                     std::to_string(!X ? 1 : (!xy ? 5 : (!K ? 9 : (!R ? 17 : 18)))) + ")");
  int rc;
  if ((rc = rs_check_search(threshold, n_hypotheses))) return rc;
  if (n_refine < 0 || n_refine > PR_MAX_REFINE)
    return fail(MVBA_ERR_BADARG, "n_refine = " + std::to_string(n_refine) + " must be in 0 .. " + std::to_string(PR_MAX_REFINE));
  if ((rc = rs_check_refit(n_refit)) || (rc = init_check_list(n_points, n_images, pt_ptr, cam_idx, n_obs)) ||
      (rc = check_camera_list(cameras, n_cameras, n_images)))
    return rc;
  std::fill(R, R + 9 * (size_t)n_cameras, NAN);
  std::fill(t, t + 3 * (size_t)n_cameras, NAN);
  PoseFit fit{R, t, n_refine};
  return robust_cameras(fit, X, n_points, pt_ptr, cam_idx, xy, n_obs, n_images, point_ok, K, cameras, n_cameras, threshold, n_hypotheses, seed, n_refit,
                        quality, n_usable, n_inliers, best, inlier, hyp_count, status, timings_ms, device);
}

int mvba_pose_refine(const double *X, int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int64_t n_obs,
                     int32_t n_images, const uint8_t *point_ok, const uint8_t *obs_ok, const double *K, const int32_t *cameras,
                     int32_t n_cameras, int32_t n_steps, double *R, double *t, double *quality, int64_t *n_usable, int32_t *status,
                     double *timings_ms, int32_t device) {
  if (n_cameras < 0) return fail(MVBA_ERR_BADARG, "n_cameras = " + std::to_string(n_cameras) + " must be >= 0");
  if (!X || !xy || !K || (n_cameras > 0 && (!R || !t)))
    return fail(MVBA_ERR_BADARG, std::string("null argument: ") + (!X ? "X" : (!xy ? "xy" : (!K ? "K" : (!R ? "R" : "t")))) + " (argument " +
                                     std::to_string(!X ? 1 : (!xy ? 5 : (!K ? 10 : (!R ? 14 : 15)))) + ")");
  if (n_steps < 0 || n_steps > PR_MAX_STEPS)
    return fail(MVBA_ERR_BADARG, "n_steps = " + std::to_string(n_steps) + " must be in 0 .. " + std::to_string(PR_MAX_STEPS));
  int rc = init_check_list(n_points, n_images, pt_ptr, cam_idx, n_obs);
  if (rc) return rc;
  const int m = n_images, nl = n_cameras;
  if ((rc = check_camera_list(cameras, n_cameras, m))) return rc;
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = 0.0;
  for (int c = 0; c < nl; ++c) {
    if (quality) quality[3 * c] = quality[3 * c + 1] = quality[3 * c + 2] = NAN;
    if (n_usable) n_usable[c] = 0;
    if (status) status[c] = 1;
  }
  if (nl == 0) return MVBA_OK;

  InitClock clk;
  ResectList list;
  resect_build_list(X, n_points, pt_ptr, cam_idx, xy, m, point_ok, obs_ok != nullptr, list);
  CamWork w;
  if ((rc = w.build(list.cam_ptr.data(), cameras, nl, START_CHUNK, nullptr))) return rc;
  // the byte mask over the listed runs: obs_ok in the sorted order; a camera needs three observations under it
  std::vector<unsigned char> msk((size_t)w.n_mask, 1);
  std::vector<int> state((size_t)nl, 0);
  int n_active = 0;
  for (int c = 0; c < nl; ++c) {
    long long n = 0;
    for (long long i = 0; i < w.lc_n[c]; ++i) {
      if (obs_ok) msk[(size_t)(w.lc_mask[c] + i)] = obs_ok[list.cm_obs[(size_t)(w.lc_start[c] + i)]] != 0;
      n += msk[(size_t)(w.lc_mask[c] + i)];
    }
    if (n_usable) n_usable[c] = n;
    if (n >= PR_MIN_REFINE_OBS) {
      state[c] = RS_ACTIVE;
      ++n_active;
    }
  }
  if (n_active == 0) {
    if (timings_ms) timings_ms[0] = clk.lap();
    return MVBA_OK;
  }

  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  DevBufs tmp;
  double *dpart = nullptr, *dS = nullptr, *dpose = nullptr, *dprev = nullptr, *dgn = nullptr;
  int *dstate = nullptr, *dgflag = nullptr;
  unsigned char *dinl = nullptr;
  if ((rc = w.upload(tmp, list, X, n_points, K))) return rc;
  const int tile = std::min(nl, 65535 * 256);
  if ((rc = tmp.alloc(&dpart, PR_NV * (size_t)w.n_ch)) || (rc = tmp.alloc(&dS, PR_NV * (size_t)tile)) || (rc = tmp.alloc(&dpose, 12 * (size_t)nl)) ||
      (rc = tmp.alloc(&dprev, 12 * (size_t)nl)) || (rc = tmp.alloc(&dgn, PG_SIZE * (size_t)nl)) || (rc = tmp.alloc(&dgflag, (size_t)nl)) ||
      (rc = tmp.alloc(&dstate, (size_t)nl)) || (rc = tmp.alloc(&dinl, (size_t)w.n_mask)))
    return rc;
  std::vector<double> pose(12 * (size_t)nl), gn(PG_SIZE * (size_t)nl);
  for (int c = 0; c < nl; ++c) {
    std::copy(R + 9 * (size_t)c, R + 9 * (size_t)c + 9, pose.begin() + 12 * (size_t)c);
    std::copy(t + 3 * (size_t)c, t + 3 * (size_t)c + 3, pose.begin() + 12 * (size_t)c + 9);
  }
  MVBA_HIP(hipMemcpy(dpose, pose.data(), sizeof(double) * 12 * nl, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dstate, state.data(), sizeof(int) * nl, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dinl, msk.data(), (size_t)w.n_mask, hipMemcpyHostToDevice));
  const double t_up = clk.lap();
  for (int c0 = 0; c0 < nl; c0 += tile) pose_iterate(w, c0, std::min(tile, nl - c0), n_steps, dstate, dinl, dinl, dpose, dprev, dgn, dgflag, dpart, dS);
  MVBA_HIP(hipGetLastError());
  MVBA_HIP(hipMemcpy(gn.data(), dgn, sizeof(double) * PG_SIZE * nl, hipMemcpyDeviceToHost));
  const double t_run = clk.lap();
  MVBA_HIP(hipMemcpy(pose.data(), dpose, sizeof(double) * 12 * nl, hipMemcpyDeviceToHost));
  for (int c = 0; c < nl; ++c) {
    if (!(state[c] & RS_ACTIVE)) continue;
    const double *rec = gn.data() + PG_SIZE * (size_t)c;
    const bool bad = rec[PG_FAIL] == 0.0;  // the first normal matrix, or an input that is not finite
    if (status) status[c] = bad ? 2 : 0;
    if (bad) continue;
    std::copy(pose.begin() + 12 * (size_t)c, pose.begin() + 12 * (size_t)c + 9, R + 9 * (size_t)c);
    std::copy(pose.begin() + 12 * (size_t)c + 9, pose.begin() + 12 * (size_t)c + 12, t + 3 * (size_t)c);
    if (quality) {
      quality[3 * c] = sqrt(rec[PG_COST0] / rec[PG_COUNT]);
      quality[3 * c + 1] = sqrt(rec[PG_COST] / rec[PG_COUNT]);
      quality[3 * c + 2] = rec[PG_STEPS];
    }
  }
  if (timings_ms) {
    timings_ms[0] = t_up;
    timings_ms[1] = t_run;
    timings_ms[2] = clk.lap();
  }
  return MVBA_OK;
}

}  // extern "C"
