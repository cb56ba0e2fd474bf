// Initial estimates for BA (mvba_triangulate, mvba_triangulate_state, mvba_resect) -- kernels and host code, gfx950.
//
// Included by mvba.hip after mvba_start.h: uses mvba_ransac_host.h's CamChunks, mvba_start.h's sym_eig_jacobi, eig_extremes, chunk_sum, init_check_list,
// init_check_cameras, upload_list, InitClock and EvLaps, and mvba.hip's mvba_handle, DevBufs, fail and MVBA_HIP.  Nothing
// here runs on the LM path, and nothing on the LM path calls into here.  
//
// Triangulation: ONE THREAD PER POINT.  A point's observations are consecutive in the CSR list, so a thread walks them in
// ascending order -- the order the sums are defined in, hence bitwise the same on every run, without atomics and without a
// cross-lane reduction -- and everything per point (the 4 x 4 moment matrix, its Jacobi, the 3 x 3 normal equations) stays in
// registers.  The degrees of the workloads this is for are small against a wave (config 3: 10 on average, config 4: 25) and
// narrowly spread (binomial), so a wave per point would idle five lanes in six and still need a fixed-order tree; the 64
// points of a wave read 64 consecutive runs of the list, every byte of a fetched line is used by the wave, and the list is
// read 2 + n_refine times of which all but the first hit in L2.  The camera matrices sit in LDS as in k_project_obs.
//
// Resection: the per-observation passes run on the device over a camera-major copy of the list (a stable counting sort on
// the HOST, inside the pass that checks the indices and drops unusable points: the list crosses PCIe afterwards anyway), cut
// into chunks of 256 observations of one camera.  One workgroup per chunk; a chunk's sums are taken by chunk_sum (a
// shuffle tree inside a wave, waves in ascending order), a camera's chunks are summed in ascending order: two runs are
// bitwise equal.  The m eigen-problems of order 12 are solved on the host by cyclic Jacobi (the same routine the
// triangulation kernel instantiates at order 4): 40 doubles per camera come back (tens of microseconds of host time each: an estimate).

namespace {

// P_k = K_k [R_k^T | -R_k^T t_k] in the order of operations of k_project_obs
__host__ __device__ __forceinline__ void init_camera_matrix(const double *Kk, const double *Rk, const double *tk, double *P) {
  double Rt[3][4];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rt[i][j] = Rk[3 * j + i];
    Rt[i][3] = -(Rt[i][0] * tk[0] + Rt[i][1] * tk[1] + Rt[i][2] * tk[2]);
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) P[4 * i + j] = Kk[3 * i] * Rt[0][j] + Kk[3 * i + 1] * Rt[1][j] + Kk[3 * i + 2] * Rt[2][j];
}

// the observations of one point: o0 .. o0 + deg - 1 of the list, or the point's row of the dense grid (cam == nullptr)
struct InitObs {
  const int *cam;
  const double2 *xy;
  long long o0;
  int deg;
  __host__ __device__ __forceinline__ int camera(int i) const { return cam ? cam[o0 + i] : i; }
  static constexpr bool MASKED = false;                                  // every observation enters the sums,
  __host__ __device__ __forceinline__ int count() const { return deg; }  // deg of them
};

// the same under a byte mask (one byte per observation of the list): the observations whose byte is set, n_used of them.
// init_point_eval and init_triangulate_point take either form; with InitObs the mask tests are discarded statements
// (if constexpr) and k_triangulate's code is, instruction for instruction, what it was.  (mvba_tri_ransac.h: the refits of
// the robust triangulation.)
struct InitObsMasked : InitObs {
  static constexpr bool MASKED = true;
  const unsigned char *mask;
  int n_used;
  __host__ __device__ __forceinline__ bool use(int i) const { return mask[o0 + i] != 0; }
  __host__ __device__ __forceinline__ int count() const { return n_used; }
};

// E = sum |pi(P X) - xy|^2 with H = sum J^T J (xx,xy,xz,yy,yz,zz) and g = sum J^T r, in ascending observation order
template <class Obs>
__host__ __device__ __forceinline__ void init_point_eval(const Obs &ob, const double *sP, const double (&X)[3], double &E,
                                                         double (&H)[6], double (&g)[3]) {
  E = 0.0;
  for (int i = 0; i < 6; ++i) H[i] = 0.0;
  for (int i = 0; i < 3; ++i) g[i] = 0.0;
  for (int i = 0; i < ob.deg; ++i) {
    if constexpr (Obs::MASKED) { if (!ob.use(i)) continue; }
    const double *P = sP + 12 * ob.camera(i);
    const double2 z = ob.xy[ob.o0 + i];
    const double p0 = X[0] * P[0] + X[1] * P[1] + X[2] * P[2] + P[3];
    const double p1 = X[0] * P[4] + X[1] * P[5] + X[2] * P[6] + P[7];
    const double p2 = X[0] * P[8] + X[1] * P[9] + X[2] * P[10] + P[11];
    const double r0 = p0 / p2 - z.x, r1 = p1 / p2 - z.y;
    const double inv = 1.0 / (p2 * p2);
    double j0[3], j1[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      j0[j] = (P[j] * p2 - p0 * P[8 + j]) * inv;
      j1[j] = (P[4 + j] * p2 - p1 * P[8 + j]) * inv;
    }
    E += r0 * r0 + r1 * r1;
    H[0] += j0[0] * j0[0] + j1[0] * j1[0];
    H[1] += j0[0] * j0[1] + j1[0] * j1[1];
    H[2] += j0[0] * j0[2] + j1[0] * j1[2];
    H[3] += j0[1] * j0[1] + j1[1] * j1[1];
    H[4] += j0[1] * j0[2] + j1[1] * j1[2];
    H[5] += j0[2] * j0[2] + j1[2] * j1[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) g[j] += j0[j] * r0 + j1[j] * r1;
  }
}

__host__ __device__ __forceinline__ bool init_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for NaN)

// d = -H^-1 g by Cholesky; false on a non-positive pivot
__host__ __device__ __forceinline__ bool init_chol3_step(const double (&H)[6], const double (&g)[3], double (&d)[3]) {
  if (!(H[0] > 0.0)) return false;
  const double l00 = sqrt(H[0]), l10 = H[1] / l00, l20 = H[2] / l00;
  const double d1 = H[3] - l10 * l10;
  if (!(d1 > 0.0)) return false;
  const double l11 = sqrt(d1), l21 = (H[4] - l20 * l10) / l11;
  const double d2 = H[5] - l20 * l20 - l21 * l21;
  if (!(d2 > 0.0)) return false;
  const double l22 = sqrt(d2);
  const double y0 = -g[0] / l00, y1 = (-g[1] - l10 * y0) / l11, y2 = (-g[2] - l20 * y0 - l21 * y1) / l22;
  d[2] = y2 / l22;
  d[1] = (y1 - l21 * d[2]) / l11;
  d[0] = (y0 - l10 * d[1] - l20 * d[2]) / l00;
  return true;
}

// One point, from all of its observations (InitObs) or from those whose mask byte is set (InitObsMasked): the linear step,
// n_refine Gauss-Newton steps, the quality figures.  Returns the status; X is NaN and q is NaN where it is not 0.  R, t: the
// cameras' poses (global memory) for the depth and the viewing rays; q is filled when want_q.
template <class Obs>
__host__ __device__ __forceinline__ int init_triangulate_point(const Obs &ob, const double *sP, const double *R, const double *t,
                                                               int n_refine, double (&X)[3], bool want_q, double (&q)[3]) {
  const double nan = NAN;
  X[0] = X[1] = X[2] = nan;
  q[0] = q[1] = q[2] = nan;
  if (ob.count() < 2) return 1;
  double A[4][4], V[4][4];
  {
    double M[10];
    for (int e = 0; e < 10; ++e) M[e] = 0.0;
    for (int i = 0; i < ob.deg; ++i) {
      if constexpr (Obs::MASKED) { if (!ob.use(i)) continue; }
      const double *P = sP + 12 * ob.camera(i);
      const double2 z = ob.xy[ob.o0 + i];
#pragma unroll
      for (int rw = 0; rw < 2; ++rw) {
        const double c = rw ? z.y : z.x;
        double r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = c * P[8 + j] - P[4 * rw + j];
        const double nr = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] /= nr;
        int e = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = a; b < 4; ++b, ++e) M[e] += r[a] * r[b];
      }
    }
    int e = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = a; b < 4; ++b, ++e) A[a][b] = A[b][a] = M[e];
  }
  sym_eig_jacobi<4>(A, V);
  double l1, l2, lmax, v[4];
  eig_extremes<4>(A, V, l1, l2, lmax, v);
  if (!(l2 > INIT_REL_PIVOT * lmax)) return 2;
  if (!(fabs(v[3]) > INIT_REL_PIVOT)) return 3;  // (|v| = 1: the point is at infinity to the precision of the eigenvector)
  double Y[3] = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
  double E = 0.0, H[6], g[3];
  if (n_refine > 0 || want_q) init_point_eval(ob, sP, Y, E, H, g);
  for (int it = 0; it < n_refine; ++it) {
    double d[3];
    if (!init_chol3_step(H, g, d)) break;
    const double Yn[3] = {Y[0] + d[0], Y[1] + d[1], Y[2] + d[2]};
    double En, Hn[6], gn[3];
    init_point_eval(ob, sP, Yn, En, Hn, gn);
    if (!(En <= E)) break;  // a step that raises the point's cost (or leaves the numbers) ends its refinement
    for (int j = 0; j < 3; ++j) { Y[j] = Yn[j]; g[j] = gn[j]; }
    for (int j = 0; j < 6; ++j) H[j] = Hn[j];
    E = En;
  }
  if (!(init_finite(Y[0]) && init_finite(Y[1]) && init_finite(Y[2]) && init_finite(E))) return 3;
  X[0] = Y[0]; X[1] = Y[1]; X[2] = Y[2];
  if (want_q) {
    double dmin = HUGE_VAL, amax = 0.0;
    for (int i = 0; i < ob.deg; ++i) {
      if constexpr (Obs::MASKED) { if (!ob.use(i)) continue; }
      const int k = ob.camera(i);
      const double *Rk = R + 9 * (size_t)k, *tk = t + 3 * (size_t)k;
      const double a0 = Y[0] - tk[0], a1 = Y[1] - tk[1], a2 = Y[2] - tk[2];
      dmin = fmin(dmin, Rk[2] * a0 + Rk[5] * a1 + Rk[8] * a2);
      for (int j = i + 1; j < ob.deg; ++j) {
        if constexpr (Obs::MASKED) { if (!ob.use(j)) continue; }
        const double *tl = t + 3 * (size_t)ob.camera(j);
        const double b0 = Y[0] - tl[0], b1 = Y[1] - tl[1], b2 = Y[2] - tl[2];
        const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
        amax = fmax(amax, atan2(sqrt(c0 * c0 + c1 * c1 + c2 * c2), a0 * b0 + a1 * b1 + a2 * b2));
      }
    }
    q[0] = sqrt(E / ob.count());
    q[1] = dmin;
    q[2] = amax;
  }
  return 0;
}

// cameras: K, R [m][9], t [m][3].  pt_ptr == nullptr: the dense grid.  keep_bad: a point whose status is not 0 keeps what X
// holds (the engine-resident form); otherwise it gets NaN.
__global__ __launch_bounds__(256) void k_triangulate(long long npts, int m, const double *__restrict__ K, const double *__restrict__ R,
                                                     const double *__restrict__ t, const long long *__restrict__ pt_ptr,
                                                     const int *__restrict__ cam_idx, const double2 *__restrict__ xy, int n_refine,
                                                     double *__restrict__ X, double *__restrict__ quality, int *__restrict__ status,
                                                     int keep_bad) {
  extern __shared__ double sP[];  // [m][12]
  for (int k = threadIdx.x; k < m; k += blockDim.x) init_camera_matrix(K + 9 * (size_t)k, R + 9 * (size_t)k, t + 3 * (size_t)k, sP + 12 * k);
  __syncthreads();
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x; a < npts; a += stride) {
    InitObs ob;
    ob.cam = pt_ptr ? cam_idx : nullptr;
    ob.xy = xy;
    ob.o0 = pt_ptr ? pt_ptr[a] : a * m;
    ob.deg = pt_ptr ? (int)(pt_ptr[a + 1] - pt_ptr[a]) : m;
    double Xa[3], q[3];
    const int st = init_triangulate_point(ob, sP, R, t, n_refine, Xa, quality != nullptr, q);
    if (st == 0 || !keep_bad) {
      X[3 * a] = Xa[0]; X[3 * a + 1] = Xa[1]; X[3 * a + 2] = Xa[2];
    }
    if (quality) { quality[3 * a] = q[0]; quality[3 * a + 1] = q[1]; quality[3 * a + 2] = q[2]; }
    if (status) status[a] = st;
  }
}

// The engine's committed cameras (f, u, v, t[3], R[9]) as K, R, t for k_triangulate.  The BA camera model
// K = [[f,0,u],[0,f,v],[0,0,f0]] projects to x / f0 (the engine's residual is p / r - x / f0 with r = f0 c3), and the engine
// holds the observations x as the caller gave them: K[2][2] = 1 here is that model with its third row divided by f0, which
// projects to x itself -- the same rows x P[2] - P[0] as (x / f0) (f0 P[2]) - P[0], and residuals in the units of xy.
__global__ __launch_bounds__(256) void k_init_cams(int m, const double *__restrict__ cam15, double *__restrict__ K,
                                                   double *__restrict__ R, double *__restrict__ t) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const double *c = cam15 + (size_t)k * CAM_IN;
  double *Kk = K + 9 * (size_t)k;
  Kk[0] = c[0]; Kk[1] = 0.0; Kk[2] = c[1];
  Kk[3] = 0.0; Kk[4] = c[0]; Kk[5] = c[2];
  Kk[6] = 0.0; Kk[7] = 0.0; Kk[8] = 1.0;
  for (int i = 0; i < 3; ++i) t[3 * (size_t)k + i] = c[3 + i];
  for (int i = 0; i < 9; ++i) R[9 * (size_t)k + i] = c[6 + i];
}

// ---- resection -----------------------------------------------------------------------------------------------------
constexpr int RS_NORM = 8;     // per camera: centroid of its points (3), their scale, centroid of its image points (2), their scale, count

// values per observation of the four passes: 0 count and first moments, 1 squared distances, 2 the 40 sums the normal
// matrix consists of, 3 the squared reprojection residual
__host__ __device__ constexpr int rs_values(int mode) { return mode == 0 ? 6 : (mode == 1 ? 2 : (mode == 2 ? 40 : 1)); }

// What one observation (point Xa, image position z) of camera k adds to pass MODE.  aux: mode 1, 2 the camera's RS_NORM
// record, mode 3 its matrix [12].
template <int MODE>
__device__ __forceinline__ void rs_pass(const double *Xa, double2 z, const double *aux, double (&v)[rs_values(MODE)]) {
  if constexpr (MODE == 0) {
    v[0] = 1.0; v[1] = Xa[0]; v[2] = Xa[1]; v[3] = Xa[2]; v[4] = z.x; v[5] = z.y;
  } else if constexpr (MODE == 1) {
    const double *nm = aux;
    const double d0 = Xa[0] - nm[0], d1 = Xa[1] - nm[1], d2 = Xa[2] - nm[2], e0 = z.x - nm[4], e1 = z.y - nm[5];
    v[0] = d0 * d0 + d1 * d1 + d2 * d2;
    v[1] = e0 * e0 + e1 * e1;
  } else if constexpr (MODE == 2) {
    const double *nm = aux;
    const double h[4] = {nm[3] * (Xa[0] - nm[0]), nm[3] * (Xa[1] - nm[1]), nm[3] * (Xa[2] - nm[2]), 1.0};
    const double x = nm[6] * (z.x - nm[4]), y = nm[6] * (z.y - nm[5]), w = x * x + y * y;
    int e = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = a; b < 4; ++b, ++e) {
        const double hh = h[a] * h[b];
        v[e] = hh; v[10 + e] = x * hh; v[20 + e] = y * hh; v[30 + e] = w * hh;
      }
  } else {
    const double *P = aux;
    const double p0 = Xa[0] * P[0] + Xa[1] * P[1] + Xa[2] * P[2] + P[3];
    const double p1 = Xa[0] * P[4] + Xa[1] * P[5] + Xa[2] * P[6] + P[7];
    const double p2 = Xa[0] * P[8] + Xa[1] * P[9] + Xa[2] * P[10] + P[11];
    const double r0 = p0 / p2 - z.x, r1 = p1 / p2 - z.y;
    v[0] = r0 * r0 + r1 * r1;
  }
}

// One workgroup per chunk (ch_cam, ch_start, ch_cnt): the chunk's sums into part[chunk][NV].  aux: mode 1, 2 the RS_NORM
// table, mode 3 the camera matrices [m][12].
template <int MODE>
__global__ __launch_bounds__(START_CHUNK) void k_resect_chunk(const int *__restrict__ ch_cam, const long long *__restrict__ ch_start,
                                                           const int *__restrict__ ch_cnt, const int *__restrict__ cm_pt,
                                                           const double2 *__restrict__ cm_xy, const double *__restrict__ X,
                                                           const double *__restrict__ aux, double *__restrict__ part) {
  constexpr int NV = rs_values(MODE);
  __shared__ double s_w[START_CHUNK / 64][NV];
  const int c = blockIdx.x, k = ch_cam[c], i = threadIdx.x;
  double v[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = 0.0;
  if (i < ch_cnt[c]) {
    const long long o = ch_start[c] + i;
    rs_pass<MODE>(X + 3 * (size_t)cm_pt[o], cm_xy[o], MODE == 0 ? aux : aux + (MODE == 3 ? 12 : RS_NORM) * (size_t)k, v);
  }
  chunk_sum<NV>(v, s_w, part + (size_t)c * NV);
}

// out[k][e] = the sum of camera k's chunk partials in ascending chunk order
__global__ __launch_bounds__(256) void k_resect_combine(int m, int nv, const int *__restrict__ cam_ch_ptr, const double *__restrict__ part,
                                                        double *__restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * nv) return;
  const int k = idx / nv, e = idx - k * nv;
  double x = 0.0;
  for (int c = cam_ch_ptr[k]; c < cam_ch_ptr[k + 1]; ++c) x += part[(size_t)c * nv + e];
  out[idx] = x;
}

// stage 0: centroids and count from the first moments S [m][6]; stage 1: the two Hartley scales from S [m][2]
__global__ __launch_bounds__(256) void k_resect_norm(int m, int stage, const double *__restrict__ S, double *__restrict__ norm) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  double *nm = norm + RS_NORM * (size_t)k;
  if (stage == 0) {
    const double *s = S + 6 * (size_t)k;
    const double n = s[0];
    nm[0] = s[1] / n; nm[1] = s[2] / n; nm[2] = s[3] / n; nm[4] = s[4] / n; nm[5] = s[5] / n;
    nm[3] = nm[6] = 0.0;
    nm[7] = n;
  } else {
    const double *s = S + 2 * (size_t)k;
    nm[3] = sqrt(3.0) / sqrt(s[0] / nm[7]);
    nm[6] = sqrt(2.0) / sqrt(s[1] / nm[7]);
  }
}

// the launch of k_triangulate on `stream`, timed by events when ms != nullptr (the stream is idle afterwards)
int launch_triangulate(hipStream_t stream, long long npts, int m, const double *K, const double *R, const double *t, const long long *pt_ptr,
                       const int *cam, const double2 *xy, int n_refine, double *X, double *quality, int *status, int keep_bad, double *ms) {
  const int lds = (int)(sizeof(double) * 12 * m);
  MVBA_HIP(hipFuncSetAttribute((const void *)k_triangulate, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const int grid = (int)std::max<long long>(1, std::min<long long>(2048, (npts + 255) / 256));
  EvLaps ev;  // (events only when the time is asked for: without them a mark records nothing)
  if (ms)
    if (int rc = ev.create(2)) return rc;
  ev.mark(stream);
  hipLaunchKernelGGL(k_triangulate, dim3(grid), dim3(256), lds, stream, npts, m, K, R, t, pt_ptr, cam, xy, n_refine, X, quality, status, keep_bad);
  hipError_t e = hipGetLastError();
  ev.mark(stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (ms) *ms = e == hipSuccess ? ev.ms(0, 1) : 0.0;
  if (e != hipSuccess) return fail(MVBA_ERR_HIP, std::string("k_triangulate: ") + hipGetErrorString(e));
  return MVBA_OK;
}

// The usable observations of a list, camera-major: a point is usable if point_ok marks it (point_ok == nullptr: if its X is
// finite); a stable counting sort by camera keeps ascending points inside a camera.  cam_ptr [m + 1] are the cameras' runs,
// cm_pt and cm_xy the point and the image position of each sorted observation, cm_obs (want_obs) its index in the caller's list.
struct ResectList {
  std::vector<long long> cam_ptr, cm_obs;
  std::vector<int> cm_pt;
  std::vector<double> cm_xy;
};

// The chunks of the listed cameras of such a list (CamChunks, chunks of START_CHUNK observations) with the list, the points
// and the chunk arrays on the device.  K (the pose calls; [n_images][9]) goes up as the listed cameras' rows, or not at all.
struct CamWork : CamChunks {
  double *dX = nullptr, *dK = nullptr;
  double2 *dxy = nullptr;
  int *dpt = nullptr, *dcams = nullptr, *dlc_n = nullptr, *dlc_ch = nullptr, *dch_cam = nullptr, *dch_cnt = nullptr;
  long long *dlc_start = nullptr, *dch_start = nullptr, *dch_mask = nullptr;

  int upload(DevBufs &tmp, const ResectList &list, const double *X, int64_t n_points, const double *K) {
    const int nl = (int)cams.size();
    const long long n_used = list.cam_ptr.back();
    int rc;
    if ((rc = tmp.alloc(&dX, 3 * (size_t)n_points)) || (rc = tmp.alloc(&dxy, (size_t)n_used)) || (rc = tmp.alloc(&dpt, (size_t)n_used)) ||
        (rc = tmp.alloc(&dcams, (size_t)nl)) || (rc = tmp.alloc(&dlc_n, (size_t)nl)) || (rc = tmp.alloc(&dlc_start, (size_t)nl)) ||
        (rc = tmp.alloc(&dlc_ch, (size_t)nl + 1)) || (rc = tmp.alloc(&dch_cam, (size_t)n_ch)) || (rc = tmp.alloc(&dch_cnt, (size_t)n_ch)) ||
        (rc = tmp.alloc(&dch_start, (size_t)n_ch)) || (rc = tmp.alloc(&dch_mask, (size_t)n_ch)))
      return rc;
    MVBA_HIP(hipMemcpy(dX, X, sizeof(double) * 3 * n_points, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dxy, list.cm_xy.data(), sizeof(double2) * n_used, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dpt, list.cm_pt.data(), sizeof(int) * n_used, hipMemcpyHostToDevice));
    if (K) {
      std::vector<double> Kl(9 * (size_t)nl);
      for (int c = 0; c < nl; ++c) std::copy(K + 9 * (size_t)cams[c], K + 9 * (size_t)cams[c] + 9, Kl.begin() + 9 * (size_t)c);
      if ((rc = tmp.alloc(&dK, 9 * (size_t)nl))) return rc;
      MVBA_HIP(hipMemcpy(dK, Kl.data(), sizeof(double) * 9 * nl, hipMemcpyHostToDevice));
    }
    MVBA_HIP(hipMemcpy(dcams, cams.data(), sizeof(int) * nl, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dlc_n, lc_n.data(), sizeof(int) * nl, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dlc_start, lc_start.data(), sizeof(long long) * nl, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dlc_ch, lc_ch.data(), sizeof(int) * (nl + 1), hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dch_cam, ch_cam.data(), sizeof(int) * n_ch, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dch_cnt, ch_cnt.data(), sizeof(int) * n_ch, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dch_start, ch_start.data(), sizeof(long long) * n_ch, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dch_mask, ch_mask.data(), sizeof(long long) * n_ch, hipMemcpyHostToDevice));
    return MVBA_OK;
  }
};

void resect_build_list(const double *X, int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int m,
                       const uint8_t *point_ok, bool want_obs, ResectList &L) {
  std::vector<uint8_t> ok((size_t)n_points);
  for (int64_t a = 0; a < n_points; ++a)
    ok[a] = point_ok ? point_ok[a] != 0 : (std::isfinite(X[3 * a]) && std::isfinite(X[3 * a + 1]) && std::isfinite(X[3 * a + 2]));
  std::vector<long long> &cam_ptr = L.cam_ptr;
  cam_ptr.assign((size_t)m + 1, 0);
  auto for_each_obs = [&](auto &&fn) {
    for (int64_t a = 0; a < n_points; ++a) {
      if (!ok[a]) continue;
      const int64_t o0 = pt_ptr ? pt_ptr[a] : a * m, o1 = pt_ptr ? pt_ptr[a + 1] : (a + 1) * m;
      for (int64_t o = o0; o < o1; ++o) fn(a, o, pt_ptr ? cam_idx[o] : (int)(o - o0));
    }
  };
  for_each_obs([&](int64_t, int64_t, int k) { ++cam_ptr[k + 1]; });
  for (int k = 0; k < m; ++k) cam_ptr[k + 1] += cam_ptr[k];
  const long long n_used = cam_ptr[m];
  L.cm_pt.resize((size_t)n_used);
  L.cm_xy.resize(2 * (size_t)n_used);
  if (want_obs) L.cm_obs.resize((size_t)n_used);
  std::vector<long long> fill(cam_ptr.begin(), cam_ptr.end() - 1);
  for_each_obs([&](int64_t a, int64_t o, int k) {
    const long long d = fill[k]++;
    L.cm_pt[d] = (int)a;
    L.cm_xy[2 * d] = xy[2 * o];
    L.cm_xy[2 * d + 1] = xy[2 * o + 1];
    if (want_obs) L.cm_obs[d] = o;
  });
}

// p (the DLT's unit eigenvector, normalised units) -> P in the units of the observations, |P[2, :3]| = 1, det P[:, :3] > 0;
// false if P is not finite.  x~ = T2 x, X~ = T3 X: P = T2^-1 P~ T3 with T2^-1 = [[1/s2, 0, cx], [0, 1/s2, cy], [0, 0, 1]],
// T3 = [[s3 I, -s3 c3], [0, 1]]; nm is the camera's RS_NORM record.
__host__ __device__ __forceinline__ bool resect_denormalise(const double *p, const double *nm, double *P) {
  const double s3 = nm[3], s2 = nm[6];
  double Q[12];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Q[4 * i + j] = s3 * p[4 * i + j];
    Q[4 * i + 3] = p[4 * i + 3] - s3 * (p[4 * i] * nm[0] + p[4 * i + 1] * nm[1] + p[4 * i + 2] * nm[2]);
  }
  for (int j = 0; j < 4; ++j) {
    P[j] = Q[j] / s2 + nm[4] * Q[8 + j];
    P[4 + j] = Q[4 + j] / s2 + nm[5] * Q[8 + j];
    P[8 + j] = Q[8 + j];
  }
  const double n3 = sqrt(P[8] * P[8] + P[9] * P[9] + P[10] * P[10]);
  const double det = P[0] * (P[5] * P[10] - P[6] * P[9]) - P[1] * (P[4] * P[10] - P[6] * P[8]) + P[2] * (P[4] * P[9] - P[5] * P[8]);
  const double sc = (det < 0.0 ? -1.0 : 1.0) / n3;
  bool ok = true;
  for (int j = 0; j < 12; ++j) {
    P[j] *= sc;
    ok = ok && init_finite(P[j]);
  }
  return ok;
}

// the sums of one camera -> its matrix (unnormalised), status and eigenvalue ratio
int resect_solve_camera(const double *S40, const double *nm, double *P, double *ratio) {
  // coincident points: a Hartley scale of sqrt(.) / sqrt(0) = inf, then inf x 0 = NaN in the sums.  The Jacobi skips a NaN
  // a_pq and eig_extremes orders NaN below nothing, so the "eigenvalues" of such a matrix would be those of its finite part:
  // degenerate here, with no ratio
  *ratio = NAN;
  for (int e = 0; e < 40; ++e)
    if (!std::isfinite(S40[e])) return 2;
  double A[12][12], V[12][12];
  for (int i = 0; i < 12; ++i)
    for (int j = 0; j < 12; ++j) A[i][j] = 0.0;
  int e = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b, ++e) {
      const double h = S40[e], xh = S40[10 + e], yh = S40[20 + e], wh = S40[30 + e];
      A[a][b] = A[b][a] = h;
      A[4 + a][4 + b] = A[4 + b][4 + a] = h;
      A[a][8 + b] = -xh; A[b][8 + a] = -xh;
      A[4 + a][8 + b] = -yh; A[4 + b][8 + a] = -yh;
      A[8 + a][8 + b] = A[8 + b][8 + a] = wh;
    }
  for (int i = 0; i < 12; ++i)
    for (int j = 0; j < i; ++j) A[i][j] = A[j][i];
  sym_eig_jacobi<12>(A, V);
  double l1, l2, lmax, p[12];
  eig_extremes<12>(A, V, l1, l2, lmax, p);
  *ratio = l1 / l2;
  if (!(l2 > INIT_REL_PIVOT * lmax)) return 2;
  return resect_denormalise(p, nm, P) ? 0 : 2;
}

}  // namespace

extern "C" {

int mvba_triangulate(const double *K, const double *R, const double *t, int32_t n_images, int64_t n_points, const int64_t *pt_ptr,
                     const int32_t *cam_idx, const double *xy, int64_t n_obs, int32_t n_refine, double *X, double *quality,
                     int32_t *status, double *timings_ms, int32_t device) {
  if (!K || !R || !t || !xy || !X)
    return fail(MVBA_ERR_BADARG, std::string("null argument: ") + (!K ? "K" : (!R ? "R" : (!t ? "t" : (!xy ? "xy" : "X")))) + " (argument " +
                                     std::to_string(!K ? 1 : (!R ? 2 : (!t ? 3 : (!xy ? 8 : 11)))) + ")");
  if (n_refine < 0) return fail(MVBA_ERR_BADARG, "n_refine = " + std::to_string(n_refine) + " must be >= 0");
  int rc = init_check_list(n_points, n_images, pt_ptr, cam_idx, n_obs);
  if (rc) return rc;
  if ((rc = init_check_cameras(n_images))) return rc;
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = 0.0;
  if (n_points == 0) return MVBA_OK;
  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  InitClock clk;
  DevBufs tmp;  // (freed on every return)
  double *dK = nullptr, *dR = nullptr, *dt = nullptr, *dX = nullptr, *dq = nullptr;
  double2 *dxy = nullptr;
  long long *dptr = nullptr;
  int *dcam = nullptr, *dst = nullptr;
  if ((rc = tmp.alloc(&dK, 9 * (size_t)n_images)) || (rc = tmp.alloc(&dR, 9 * (size_t)n_images)) || (rc = tmp.alloc(&dt, 3 * (size_t)n_images)) ||
      (rc = tmp.alloc(&dX, 3 * (size_t)n_points)))
    return rc;
  if (quality && (rc = tmp.alloc(&dq, 3 * (size_t)n_points))) return rc;
  if (status && (rc = tmp.alloc(&dst, (size_t)n_points))) return rc;
  MVBA_HIP(hipMemcpy(dK, K, sizeof(double) * 9 * n_images, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dR, R, sizeof(double) * 9 * n_images, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dt, t, sizeof(double) * 3 * n_images, hipMemcpyHostToDevice));
  if ((rc = upload_list(tmp, n_points, n_obs, pt_ptr, cam_idx, xy, &dptr, &dcam, &dxy))) return rc;
  if (timings_ms) timings_ms[0] = clk.lap();
  double ms = 0.0;
  if ((rc = launch_triangulate(nullptr, n_points, n_images, dK, dR, dt, dptr, dcam, dxy, n_refine, dX, dq, dst, 0, timings_ms ? &ms : nullptr))) return rc;
  if (timings_ms) { timings_ms[1] = ms; clk.lap(); }
  MVBA_HIP(hipMemcpy(X, dX, sizeof(double) * 3 * n_points, hipMemcpyDeviceToHost));
  if (quality) MVBA_HIP(hipMemcpy(quality, dq, sizeof(double) * 3 * n_points, hipMemcpyDeviceToHost));
  if (status) MVBA_HIP(hipMemcpy(status, dst, sizeof(int) * n_points, hipMemcpyDeviceToHost));
  if (timings_ms) timings_ms[2] = clk.lap();
  return MVBA_OK;
}

int mvba_triangulate_state(mvba_handle *h, int32_t n_refine, double *quality, int32_t *status, double *timings_ms) {
  if (!h) return fail(MVBA_ERR_BADARG, "null argument: h (argument 1)");
  if (n_refine < 0) return fail(MVBA_ERR_BADARG, "n_refine = " + std::to_string(n_refine) + " must be >= 0");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set: the cameras to triangulate from are the committed ones");
  if (h->n_held)
    return fail(MVBA_ERR_STATE, "mvba_triangulate_state: " + std::to_string(h->n_held) + " points are held (mvba_set_point_hold) and would be "
                                "replaced by their triangulation: clear the mask first (mvba_set_point_hold(h, NULL))");
  int rc = init_check_cameras(h->m);
  if (rc) return rc;
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = 0.0;
  MVBA_HIP(hipSetDevice(h->device));
  if (!h->d_init_cams && (rc = h->mem.alloc(&h->d_init_cams, 21 * (size_t)h->m))) return rc;
  double *dK = h->d_init_cams, *dR = dK + 9 * (size_t)h->m, *dt = dR + 9 * (size_t)h->m;
  DevBufs tmp;
  double *dq = nullptr;
  int *dst = nullptr;
  if (quality && (rc = tmp.alloc(&dq, 3 * (size_t)std::max<long long>(h->N, 1)))) return rc;
  if (status && (rc = tmp.alloc(&dst, (size_t)std::max<long long>(h->N, 1)))) return rc;
  hipLaunchKernelGGL(k_init_cams, dim3((h->m + 255) / 256), dim3(256), 0, h->stream, h->m, h->d_cam15[h->cur], dK, dR, dt);
  MVBA_HIP(hipGetLastError());
  h->linearized = false; h->have_trial = false;  // (as mvba_set_params: the committed points change)
  if (h->N == 0) return sync_and_drain(h);
  double ms = 0.0;
  if ((rc = launch_triangulate(h->stream, h->N, h->m, dK, dR, dt, h->d_pt_ptr, h->d_cam, h->d_xy, n_refine, h->d_X[h->cur], dq, dst, 1,
                               timings_ms ? &ms : nullptr)))
    return rc;
  drain_events(h);
  InitClock clk;
  if (quality) MVBA_HIP(hipMemcpy(quality, dq, sizeof(double) * 3 * h->N, hipMemcpyDeviceToHost));
  if (status) MVBA_HIP(hipMemcpy(status, dst, sizeof(int) * h->N, hipMemcpyDeviceToHost));
  if (timings_ms) { timings_ms[1] = ms; timings_ms[2] = clk.lap(); }
  return MVBA_OK;
}

int mvba_resect(const double *X, int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int64_t n_obs,
                int32_t n_images, const uint8_t *point_ok, double *P, double *quality, int32_t *status, double *timings_ms,
                int32_t device) {
  if (!X || !xy || !P)
    return fail(MVBA_ERR_BADARG, std::string("null argument: ") + (!X ? "X" : (!xy ? "xy" : "P")) + " (argument " + std::to_string(!X ? 1 : (!xy ? 5 : 9)) + ")");
  int rc = init_check_list(n_points, n_images, pt_ptr, cam_idx, n_obs);
  if (rc) return rc;
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = 0.0;
  const int m = n_images;
  InitClock clk;
  ResectList list;
  resect_build_list(X, n_points, pt_ptr, cam_idx, xy, m, point_ok, false, list);
  const std::vector<long long> &cam_ptr = list.cam_ptr;
  CamWork w;  // (every camera: list position = camera)
  if ((rc = w.build(cam_ptr.data(), nullptr, m, START_CHUNK, nullptr))) return rc;
  const int n_ch = w.n_ch;
  std::vector<double> Pm(12 * (size_t)m, NAN), norm(RS_NORM * (size_t)m, 0.0), S40(40 * (size_t)m, 0.0), Sr((size_t)m, 0.0), ratio((size_t)m, NAN);
  std::vector<int> st((size_t)m, 1);
  double kernel_ms = 0.0;
  if (n_ch > 0) {
    if (device >= 0) MVBA_HIP(hipSetDevice(device));
    DevBufs tmp;
    double *dpart = nullptr, *dS = nullptr, *dnorm = nullptr, *dP = nullptr;
    if ((rc = w.upload(tmp, list, X, n_points, nullptr)) || (rc = tmp.alloc(&dpart, 40 * (size_t)n_ch)) || (rc = tmp.alloc(&dS, 40 * (size_t)m)) ||
        (rc = tmp.alloc(&dnorm, RS_NORM * (size_t)m)) || (rc = tmp.alloc(&dP, 12 * (size_t)m)))
      return rc;
    if (timings_ms) timings_ms[0] = clk.lap();
    EvLaps ev;
    if ((rc = ev.create(4))) return rc;
    const dim3 gm((m + 255) / 256), b256(256);
    auto combine = [&](int nv) { hipLaunchKernelGGL(k_resect_combine, dim3((m * nv + 255) / 256), b256, 0, 0, m, nv, w.dlc_ch, dpart, dS); };
    ev.mark();
    hipLaunchKernelGGL(k_resect_chunk<0>, dim3(n_ch), dim3(START_CHUNK), 0, 0, w.dch_cam, w.dch_start, w.dch_cnt, w.dpt, w.dxy, w.dX, (const double *)nullptr, dpart);
    combine(6);
    hipLaunchKernelGGL(k_resect_norm, gm, b256, 0, 0, m, 0, dS, dnorm);
    hipLaunchKernelGGL(k_resect_chunk<1>, dim3(n_ch), dim3(START_CHUNK), 0, 0, w.dch_cam, w.dch_start, w.dch_cnt, w.dpt, w.dxy, w.dX, dnorm, dpart);
    combine(2);
    hipLaunchKernelGGL(k_resect_norm, gm, b256, 0, 0, m, 1, dS, dnorm);
    hipLaunchKernelGGL(k_resect_chunk<2>, dim3(n_ch), dim3(START_CHUNK), 0, 0, w.dch_cam, w.dch_start, w.dch_cnt, w.dpt, w.dxy, w.dX, dnorm, dpart);
    combine(40);
    ev.mark();
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(S40.data(), dS, sizeof(double) * 40 * m, hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(norm.data(), dnorm, sizeof(double) * RS_NORM * m, hipMemcpyDeviceToHost));
    for (int k = 0; k < m; ++k) {
      if (cam_ptr[k + 1] - cam_ptr[k] < 6) continue;  // status 1
      st[k] = resect_solve_camera(S40.data() + 40 * (size_t)k, norm.data() + RS_NORM * (size_t)k, Pm.data() + 12 * (size_t)k, &ratio[k]);
      if (st[k])
        for (int j = 0; j < 12; ++j) Pm[12 * (size_t)k + j] = NAN;
    }
    MVBA_HIP(hipMemcpy(dP, Pm.data(), sizeof(double) * 12 * m, hipMemcpyHostToDevice));
    ev.mark();
    hipLaunchKernelGGL(k_resect_chunk<3>, dim3(n_ch), dim3(START_CHUNK), 0, 0, w.dch_cam, w.dch_start, w.dch_cnt, w.dpt, w.dxy, w.dX, dP, dpart);
    combine(1);
    ev.mark();
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(Sr.data(), dS, sizeof(double) * m, hipMemcpyDeviceToHost));
    kernel_ms = ev.ms(0, 1) + ev.ms(2, 3);
  }
  for (int k = 0; k < m; ++k) {
    for (int j = 0; j < 12; ++j) P[12 * (size_t)k + j] = Pm[12 * (size_t)k + j];
    if (status) status[k] = st[k];
    if (quality) {
      quality[2 * k] = st[k] == 0 ? sqrt(Sr[k] / (double)(cam_ptr[k + 1] - cam_ptr[k])) : NAN;
      quality[2 * k + 1] = st[k] == 1 ? NAN : ratio[k];
    }
  }
  if (timings_ms) {
    timings_ms[1] = kernel_ms;
    timings_ms[2] = lap_rest(clk.lap(), kernel_ms);  // the copies back, the host's eigen-solves and the second upload of P
  }
  return MVBA_OK;
}

}  // extern "C"
