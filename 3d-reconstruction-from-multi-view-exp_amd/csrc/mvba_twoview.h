// Starting a reconstruction from two views (mvba_covisibility, mvba_two_view) -- kernels and host code, gfx950.
//
// Included by mvba.hip after mvba_start.h and mvba_init.h: uses mvba_start.h's sym_eig_jacobi, eig_extremes, chunk_sum, the
// list and pair checks, upload_list, InitClock and EvLaps, and mvba.hip's DevBufs, fail and MVBA_HIP.  Nothing here runs on
// the LM path.  
//
// Co-visibility: ONE THREAD PER POINT walks the pairs of its own camera run (deg^2 / 2 increments) into an m x m table of
// integer counters -- integer sums are exact in any order, so these are atomics: a per-workgroup table in LDS that is flushed
// once while m^2 x 4 bytes fit 64 KiB (m <= 128), 64-bit atomics on device memory beyond.  Only k <= l is counted; the host
// mirrors the triangle.
//
// Epipolar moments: one workgroup of 256 threads takes 256 consecutive points for one pair (blockIdx.y: the pair inside the
// launch's tile of pairs).  A thread finds k and l in its point's ascending camera run by two binary searches, forms its
// values (tv_pass, or zeros) and the workgroup sums them by chunk_sum; k_twoview_combine adds a pair's chunk
// partials in an order that depends on the chunk count alone.  No floating-point atomics: two runs are bitwise equal.  The
// eigen-problems of order 9 are solved on the host (sym_eig_jacobi<9>), as mvba_resect solves its own of order 12.

namespace {

constexpr int TV_NORM = 8;                      // per pair: centroid in k (2), scale in k, centroid in l (2), scale in l, count, unused
constexpr int TV_MIN_SHARED = 8;                // the linear solution needs 8 rows
constexpr size_t TV_PART_BYTES = 128u << 20;    // chunk partials of one launch: pairs are tiled to stay under this
constexpr int CV_LDS_CAMERAS = 128;             // m^2 x 4 bytes <= 64 KiB: the co-visibility table lives in LDS

// values per shared point of the four passes: 0 count and first moments, 1 squared distances to the centroids, 2 the 45
// unique products of the epipolar row, 3 the squared Sampson distance, 4 the 45 unique products of the two homography
// (DLT) rows, summed over the two (mvba_homography.h)
__host__ __device__ constexpr int tv_values(int mode) { return mode == 0 ? 5 : (mode == 1 ? 2 : (mode == 2 || mode == 4 ? 45 : 1)); }
// doubles per pair of what a pass reads besides the point: 0 nothing, 1 and 2 the TV_NORM record, 3 F
__host__ __device__ constexpr int tv_aux(int mode) { return mode == 0 ? 0 : (mode == 3 ? 9 : TV_NORM); }

__global__ __launch_bounds__(256) void k_covisibility(long long npts, int m, const long long *__restrict__ pt_ptr,
                                                      const int *__restrict__ cam_idx, unsigned long long *__restrict__ count,
                                                      int use_lds) {
  extern __shared__ unsigned int s_cv[];  // [m][m] when use_lds (a workgroup sees fewer than 2^31 points: 32 bits hold its counts)
  if (use_lds) {
    for (int e = threadIdx.x; e < m * m; e += blockDim.x) s_cv[e] = 0u;
    __syncthreads();
  }
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x; a < npts; a += stride) {
    const long long o0 = pt_ptr ? pt_ptr[a] : a * m;
    const int deg = pt_ptr ? (int)(pt_ptr[a + 1] - pt_ptr[a]) : m;
    for (int i = 0; i < deg; ++i) {
      const int ci = pt_ptr ? cam_idx[o0 + i] : i;
      for (int j = i; j < deg; ++j) {
        const int cj = pt_ptr ? cam_idx[o0 + j] : j;
        const size_t e = (size_t)min(ci, cj) * m + max(ci, cj);
        if (use_lds) atomicAdd(&s_cv[e], 1u);
        else atomicAdd(&count[e], 1ull);
      }
    }
  }
  if (use_lds) {
    __syncthreads();
    for (int e = threadIdx.x; e < m * m; e += blockDim.x) {
      const unsigned int v = s_cv[e];
      if (v) atomicAdd(&count[e], (unsigned long long)v);
    }
  }
}

// the observation of camera c in the ascending run cam[o0 .. o0 + deg), or -1; cam == nullptr: the dense grid
__device__ __forceinline__ long long tv_find(const int *__restrict__ cam, long long o0, int deg, int c) {
  if (!cam) return o0 + c;
  int lo = 0, hi = deg;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cam[o0 + mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return (lo < deg && cam[o0 + lo] == c) ? o0 + lo : -1;
}

// does point a see both cameras of the pair?  (its two observations in ok, ol)
__device__ __forceinline__ bool rs_shared(long long a, long long npts, int m, const long long *__restrict__ pt_ptr,
                                          const int *__restrict__ cam_idx, int k, int l, long long &ok, long long &ol) {
  ok = ol = -1;
  if (a < npts) {
    const long long o0 = pt_ptr ? pt_ptr[a] : a * m;
    const int deg = pt_ptr ? (int)(pt_ptr[a + 1] - pt_ptr[a]) : m;
    const int *cam = pt_ptr ? cam_idx : nullptr;
    ok = tv_find(cam, o0, deg, k);
    if (ok >= 0) ol = tv_find(cam, o0, deg, l);
  }
  return ok >= 0 && ol >= 0;
}

// the squared Sampson distance of (xk, yk) in k and (xl, yl) in l under F
__device__ __forceinline__ double rs_sampson(const double *F, double xk, double yk, double xl, double yl) {
  const double f0 = F[0] * xk + F[1] * yk + F[2], f1 = F[3] * xk + F[4] * yk + F[5], f2 = F[6] * xk + F[7] * yk + F[8];
  const double g0 = F[0] * xl + F[3] * yl + F[6], g1 = F[1] * xl + F[4] * yl + F[7];
  const double r = xl * f0 + yl * f1 + f2;
  return r * r / (f0 * f0 + f1 * f1 + g0 * g0 + g1 * g1);
}

// the epipolar row of one correspondence in the normalised coordinates of the pair's TV_NORM record nm: r . f^ = 0
__device__ __forceinline__ void tv_row(const double *nm, double zkx, double zky, double zlx, double zly, double (&r)[9]) {
  const double xk = nm[2] * (zkx - nm[0]), yk = nm[2] * (zky - nm[1]);
  const double xl = nm[5] * (zlx - nm[3]), yl = nm[5] * (zly - nm[4]);
  r[0] = xl * xk; r[1] = xl * yk; r[2] = xl; r[3] = yl * xk; r[4] = yl * yk; r[5] = yl; r[6] = xk; r[7] = yk; r[8] = 1.0;
}

// the two rows of one correspondence x_l ~ H^ x_k in the normalised coordinates of the pair's TV_NORM record nm:
// r1 . h^ = r2 . h^ = 0 (the third row of the cross product is a combination of the two)
__device__ __forceinline__ void hg_rows(const double *nm, double zkx, double zky, double zlx, double zly, double (&r1)[9], double (&r2)[9]) {
  const double xk = nm[2] * (zkx - nm[0]), yk = nm[2] * (zky - nm[1]);
  const double xl = nm[5] * (zlx - nm[3]), yl = nm[5] * (zly - nm[4]);
  r1[0] = xk; r1[1] = yk; r1[2] = 1.0; r1[3] = r1[4] = r1[5] = 0.0; r1[6] = -xl * xk; r1[7] = -xl * yk; r1[8] = -xl;
  r2[0] = r2[1] = r2[2] = 0.0; r2[3] = xk; r2[4] = yk; r2[5] = 1.0; r2[6] = -yl * xk; r2[7] = -yl * yk; r2[8] = -yl;
}

// The values of one shared point, (xk, yk) in k and (xl, yl) in l, in pass MODE.  aux (of the pair): mode 1, 2 its TV_NORM
// record, mode 3 F [9], mode 4 its TV_NORM record (tv_aux doubles).
template <int MODE>
__device__ __forceinline__ void tv_pass(double xk, double yk, double xl, double yl, const double *aux, double (&v)[tv_values(MODE)]) {
  if constexpr (MODE == 0) {
    v[0] = 1.0; v[1] = xk; v[2] = yk; v[3] = xl; v[4] = yl;
  } else if constexpr (MODE == 1) {
    const double d0 = xk - aux[0], d1 = yk - aux[1], e0 = xl - aux[3], e1 = yl - aux[4];
    v[0] = d0 * d0 + d1 * d1;
    v[1] = e0 * e0 + e1 * e1;
  } else if constexpr (MODE == 2) {
    double r[9];
    tv_row(aux, xk, yk, xl, yl, r);
    int e = 0;
#pragma unroll
    for (int b = 0; b < 9; ++b)
#pragma unroll
      for (int c = b; c < 9; ++c, ++e) v[e] = r[b] * r[c];
  } else if constexpr (MODE == 4) {
    double r1[9], r2[9];
    hg_rows(aux, xk, yk, xl, yl, r1, r2);
    int e = 0;
#pragma unroll
    for (int b = 0; b < 9; ++b)
#pragma unroll
      for (int c = b; c < 9; ++c, ++e) v[e] = r1[b] * r1[c] + r2[b] * r2[c];
  } else {
    v[0] = rs_sampson(aux, xk, yk, xl, yl);
  }
}

// F = T_l^T F^ T_k with T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]: f the row-major F^, nm the pair's TV_NORM record
__host__ __device__ __forceinline__ void tv_denormalise(const double *nm, const double *f, double *F) {
  const double ckx = nm[0], cky = nm[1], sk = nm[2], clx = nm[3], cly = nm[4], sl = nm[5];
  double Q[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Q[i][0] = sk * f[3 * i];
    Q[i][1] = sk * f[3 * i + 1];
    Q[i][2] = f[3 * i + 2] - sk * (ckx * f[3 * i] + cky * f[3 * i + 1]);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    F[j] = sl * Q[0][j];
    F[3 + j] = sl * Q[1][j];
    F[6 + j] = Q[2][j] - sl * (clx * Q[0][j] + cly * Q[1][j]);
  }
}

// H = T_b^-1 H^ T_a with T^-1 = [[1/s, 0, cx], [0, 1/s, cy], [0, 0, 1]]: h the row-major H^ that maps the normalised points of
// image a to those of image b; na, nb = (cx, cy, s) of the two images (nm, nm + 3 of a TV_NORM record, or the other way round
// for the inverse map)
__host__ __device__ __forceinline__ void hg_denormalise(const double *na, const double *nb, const double *h, double *H) {
  double Q[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Q[i][0] = na[2] * h[3 * i];
    Q[i][1] = na[2] * h[3 * i + 1];
    Q[i][2] = h[3 * i + 2] - na[2] * (na[0] * h[3 * i] + na[1] * h[3 * i + 1]);
  }
  const double inv = 1.0 / nb[2];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    H[j] = inv * Q[0][j] + nb[0] * Q[2][j];
    H[3 + j] = inv * Q[1][j] + nb[1] * Q[2][j];
    H[6 + j] = Q[2][j];
  }
}

// One workgroup per (chunk of 256 points, pair of the tile): the chunk's sums over the points both cameras see into
// part[pair][chunk][NV].  aux (per pair of the tile): mode 1, 2 the TV_NORM table, mode 3 F [9].
template <int MODE>
__global__ __launch_bounds__(START_CHUNK) void k_twoview_chunk(long long npts, int m, const long long *__restrict__ pt_ptr,
                                                            const int *__restrict__ cam_idx, const double2 *__restrict__ xy,
                                                            const int *__restrict__ pairs, const double *__restrict__ aux,
                                                            double *__restrict__ part) {
  constexpr int NV = tv_values(MODE);
  __shared__ double s_w[START_CHUNK / 64][NV];
  const int p = blockIdx.y, i = threadIdx.x;
  const long long a = (long long)blockIdx.x * START_CHUNK + i;
  const double *nm = aux + tv_aux(MODE) * (size_t)p;
  double v[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = 0.0;
  long long ok, ol;
  rs_shared(a, npts, m, pt_ptr, cam_idx, pairs[2 * p], pairs[2 * p + 1], ok, ol);
  if (ok >= 0 && ol >= 0) {
    const double2 zk = xy[ok], zl = xy[ol];
    tv_pass<MODE>(zk.x, zk.y, zl.x, zl.y, nm, v);
  }
  chunk_sum<NV>(v, s_w, part + ((size_t)p * gridDim.x + blockIdx.x) * NV);
}

// out[p][e] = the sum of pair p's chunk partials: one wave per (p, e); lane j adds the chunks j, j + 64, ... in ascending
// order, then the lanes are added by the shuffle tree -- an order that the chunk count fixes
__global__ __launch_bounds__(256) void k_twoview_combine(int n_pairs, int nv, int n_chunks, const double *__restrict__ part,
                                                         double *__restrict__ out, int out_stride) {
  const long long w = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (w >= (long long)n_pairs * nv) return;  // (whole waves leave: the shuffles below see all 64 lanes)
  const int p = (int)(w / nv), e = (int)(w - (long long)p * nv), lane = threadIdx.x & 63;
  double x = 0.0;
  for (int c = lane; c < n_chunks; c += 64) x += part[((size_t)p * n_chunks + c) * nv + e];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  if (lane == 0) out[(size_t)p * out_stride + e] = x;
}

// stage 0: count and centroids from the first moments S [n_pairs][5]; stage 1: the two Hartley scales from S [n_pairs][2]
__global__ __launch_bounds__(256) void k_twoview_norm(int n_pairs, int stage, const double *__restrict__ S, int s_stride,
                                                      double *__restrict__ norm) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  double *nm = norm + TV_NORM * (size_t)p;
  const double *s = S + (size_t)s_stride * p;
  if (stage == 0) {
    const double n = s[0];
    nm[0] = s[1] / n; nm[1] = s[2] / n; nm[3] = s[3] / n; nm[4] = s[4] / n;
    nm[2] = nm[5] = nm[7] = 0.0;
    nm[6] = n;
  } else {
    nm[2] = sqrt(2.0) / sqrt(s[0] / nm[6]);
    nm[5] = sqrt(2.0) / sqrt(s[1] / nm[6]);
  }
}

// the 45 sums of one pair -> F (normalisation undone, |F| = 1, largest entry positive), status and lambda_1 / lambda_2
int twoview_solve_pair(const double *S45, const double *nm, double *F, double *ratio) {
  *ratio = NAN;
  for (int e = 0; e < 45; ++e)  // coincident image points in k or l (an infinite Hartley scale): as resect_solve_camera
    if (!std::isfinite(S45[e])) return 2;
  double A[9][9], V[9][9];
  int e = 0;
  for (int b = 0; b < 9; ++b)
    for (int c = b; c < 9; ++c, ++e) A[b][c] = A[c][b] = S45[e];
  sym_eig_jacobi<9>(A, V);
  double l1, l2, lmax, f[9];
  eig_extremes<9>(A, V, l1, l2, lmax, f);
  *ratio = l1 / l2;
  if (!(l2 > INIT_REL_PIVOT * lmax)) return 2;
  // rank 2: F^ <- F^ (I - v v^T), v the right singular vector of the smallest singular value (eigenvector of F^^T F^)
  double G[3][3], W[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) G[i][j] = f[i] * f[j] + f[3 + i] * f[3 + j] + f[6 + i] * f[6 + j];
  sym_eig_jacobi<3>(G, W);
  double m1, m2, mmax, v[3];
  eig_extremes<3>(G, W, m1, m2, mmax, v);
  double H[9];
  for (int i = 0; i < 3; ++i) {
    const double fv = f[3 * i] * v[0] + f[3 * i + 1] * v[1] + f[3 * i + 2] * v[2];
    for (int j = 0; j < 3; ++j) H[3 * i + j] = f[3 * i + j] - fv * v[j];
  }
  tv_denormalise(nm, H, F);
  double nrm = 0.0, big = 0.0;
  for (int j = 0; j < 9; ++j) {
    nrm += F[j] * F[j];
    if (fabs(F[j]) > fabs(big)) big = F[j];
  }
  const double sc = (big < 0.0 ? -1.0 : 1.0) / sqrt(nrm);
  bool ok = true;
  for (int j = 0; j < 9; ++j) {
    F[j] *= sc;
    ok = ok && std::isfinite(F[j]);
  }
  return ok ? 0 : 2;
}

// the 45 sums of one pair (tv_pass mode 4) -> H = T_l^-1 H^ T_k (|H| = 1, largest entry positive), status and lambda_1 /
// lambda_2: twoview_solve_pair without the rank-2 step
int homography_solve_pair(const double *S45, const double *nm, double *H, double *ratio) {
  *ratio = NAN;
  for (int e = 0; e < 45; ++e)
    if (!std::isfinite(S45[e])) return 2;
  double A[9][9], V[9][9];
  int e = 0;
  for (int b = 0; b < 9; ++b)
    for (int c = b; c < 9; ++c, ++e) A[b][c] = A[c][b] = S45[e];
  sym_eig_jacobi<9>(A, V);
  double l1, l2, lmax, h[9];
  eig_extremes<9>(A, V, l1, l2, lmax, h);
  *ratio = l1 / l2;
  if (!(l2 > INIT_REL_PIVOT * lmax)) return 2;
  hg_denormalise(nm, nm + 3, h, H);
  return hg_unit(H) ? 0 : 2;
}

// pairs per launch: the tile's device bytes stay under TV_PART_BYTES, its count within gridDim.y
int tv_pair_tile(int n_pairs, size_t bytes_per_pair) {
  return (int)std::max<long long>(1, std::min<long long>(std::min<long long>(n_pairs, 65535), (long long)(TV_PART_BYTES / bytes_per_pair)));
}

// the launch of k_twoview_combine over the cnt pairs of a tile
void tv_combine(int cnt, int nv, long long n_ch, const double *part, double *out, int stride) {
  hipLaunchKernelGGL(k_twoview_combine, dim3((unsigned)(((long long)cnt * nv + 3) / 4)), dim3(256), 0, 0, cnt, nv, (int)n_ch, part, out, stride);
}

}  // namespace

extern "C" {

int mvba_covisibility(int64_t n_points, int32_t n_images, const int64_t *pt_ptr, const int32_t *cam_idx, int64_t n_obs,
                      int64_t *count, double *timings_ms, int32_t device) {
  if (!count) return fail(MVBA_ERR_BADARG, "null argument: count (argument 6)");
  int rc = init_check_list(n_points, n_images, pt_ptr, cam_idx, n_obs);
  if (rc) return rc;
  if ((rc = init_check_cameras(n_images))) return rc;
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = 0.0;
  const int m = n_images;
  const size_t mm = (size_t)m * m;
  for (size_t e = 0; e < mm; ++e) count[e] = 0;
  if (n_points == 0) return MVBA_OK;
  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  InitClock clk;
  DevBufs tmp;
  long long *dptr = nullptr;
  int *dcam = nullptr;
  unsigned long long *dcount = nullptr;
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters come back as they are");
  if ((rc = tmp.alloc(&dcount, mm))) return rc;
  MVBA_HIP(hipMemset(dcount, 0, sizeof(unsigned long long) * mm));
  if ((rc = upload_list(tmp, n_points, n_obs, pt_ptr, cam_idx, nullptr, &dptr, &dcam, nullptr))) return rc;
  if (timings_ms) timings_ms[0] = clk.lap();
  EvLaps ev;
  if ((rc = ev.create(2))) return rc;
  const int use_lds = m <= CV_LDS_CAMERAS;
  const int lds = use_lds ? (int)(sizeof(unsigned int) * mm) : 0;
  MVBA_HIP(hipFuncSetAttribute((const void *)k_covisibility, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const int grid = (int)std::max<long long>(1, std::min<long long>(2048, (n_points + 255) / 256));
  ev.mark();
  hipLaunchKernelGGL(k_covisibility, dim3(grid), dim3(256), lds, 0, (long long)n_points, m, dptr, dcam, dcount, use_lds);
  ev.mark();
  MVBA_HIP(hipGetLastError());
  MVBA_HIP(hipMemcpy(count, dcount, sizeof(int64_t) * mm, hipMemcpyDeviceToHost));
  for (int k = 0; k < m; ++k)
    for (int l = k + 1; l < m; ++l) count[(size_t)l * m + k] = count[(size_t)k * m + l];
  if (timings_ms) {
    timings_ms[1] = ev.ms(0, 1);
    timings_ms[2] = lap_rest(clk.lap(), timings_ms[1]);
  }
  return MVBA_OK;
}

int mvba_two_view(int64_t n_points, int32_t n_images, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int64_t n_obs,
                  const int32_t *pairs, int32_t n_pairs, double *F, double *quality, int64_t *n_shared, int32_t *status,
                  double *timings_ms, int32_t device) {
  if (n_pairs < 0) return fail(MVBA_ERR_BADARG, "n_pairs = " + std::to_string(n_pairs) + " must be >= 0");
  if (!xy || (n_pairs > 0 && (!pairs || !F)))
    return fail(MVBA_ERR_BADARG, std::string("null argument: ") + (!xy ? "xy" : (!pairs ? "pairs" : "F")) + " (argument " +
                                     std::to_string(!xy ? 5 : (!pairs ? 7 : 9)) + ")");
  int rc = init_check_list(n_points, n_images, pt_ptr, cam_idx, n_obs);
  if (rc) return rc;
  if ((rc = init_check_cameras(n_images))) return rc;
  if ((rc = check_pairs(pairs, n_pairs, n_images))) return rc;
  if ((rc = check_ascending(n_points, pt_ptr, cam_idx))) return rc;
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = 0.0;
  const int np = n_pairs;
  std::vector<double> Fm(9 * (size_t)np, NAN), S((size_t)np * 45, 0.0), norm(TV_NORM * (size_t)np, 0.0), Sr((size_t)np, 0.0), ratio((size_t)np, NAN);
  std::vector<int> st((size_t)np, 1);
  if (np > 0 && n_points > 0) {
    if (device >= 0) MVBA_HIP(hipSetDevice(device));
    InitClock clk;
    const long long n_ch = (n_points + START_CHUNK - 1) / START_CHUNK;
    const int tile = tv_pair_tile(np, sizeof(double) * 45 * (size_t)n_ch);
    DevBufs tmp;
    double2 *dxy = nullptr;
    long long *dptr = nullptr;
    int *dcam = nullptr, *dpairs = nullptr;
    double *dpart = nullptr, *dS = nullptr, *dnorm = nullptr, *dF = nullptr, *dS1 = nullptr;
    if ((rc = upload_list(tmp, n_points, n_obs, pt_ptr, cam_idx, xy, &dptr, &dcam, &dxy)) || (rc = tmp.alloc(&dpairs, 2 * (size_t)np)) || (rc = tmp.alloc(&dpart, 45 * (size_t)n_ch * tile)) ||
        (rc = tmp.alloc(&dS, 45 * (size_t)np)) || (rc = tmp.alloc(&dS1, 5 * (size_t)tile)) || (rc = tmp.alloc(&dnorm, TV_NORM * (size_t)np)) ||
        (rc = tmp.alloc(&dF, 9 * (size_t)np)))
      return rc;
    MVBA_HIP(hipMemcpy(dpairs, pairs, sizeof(int) * 2 * np, hipMemcpyHostToDevice));
    if (timings_ms) timings_ms[0] = clk.lap();
    EvLaps ev;
    if ((rc = ev.create(4))) return rc;
    const dim3 b256(256);
    auto combine = [&](int cnt, int nv, double *out, int stride) { tv_combine(cnt, nv, n_ch, dpart, out, stride); };
    ev.mark();
    for (int p0 = 0; p0 < np; p0 += tile) {
      const int cnt = std::min(tile, np - p0);
      const dim3 grid((unsigned)n_ch, (unsigned)cnt), gp((cnt + 255) / 256);
      const int *tp = dpairs + 2 * (size_t)p0;
      double *tn = dnorm + TV_NORM * (size_t)p0;
      hipLaunchKernelGGL(k_twoview_chunk<0>, grid, dim3(START_CHUNK), 0, 0, (long long)n_points, n_images, dptr, dcam, dxy, tp, (const double *)nullptr, dpart);
      combine(cnt, 5, dS1, 5);
      hipLaunchKernelGGL(k_twoview_norm, gp, b256, 0, 0, cnt, 0, dS1, 5, tn);
      hipLaunchKernelGGL(k_twoview_chunk<1>, grid, dim3(START_CHUNK), 0, 0, (long long)n_points, n_images, dptr, dcam, dxy, tp, tn, dpart);
      combine(cnt, 2, dS1, 2);
      hipLaunchKernelGGL(k_twoview_norm, gp, b256, 0, 0, cnt, 1, dS1, 2, tn);
      hipLaunchKernelGGL(k_twoview_chunk<2>, grid, dim3(START_CHUNK), 0, 0, (long long)n_points, n_images, dptr, dcam, dxy, tp, tn, dpart);
      combine(cnt, 45, dS + 45 * (size_t)p0, 45);
    }
    ev.mark();
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(S.data(), dS, sizeof(double) * 45 * np, hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(norm.data(), dnorm, sizeof(double) * TV_NORM * np, hipMemcpyDeviceToHost));
    for (int p = 0; p < np; ++p) {
      if (!(norm[TV_NORM * (size_t)p + 6] >= TV_MIN_SHARED)) continue;  // status 1
      st[p] = twoview_solve_pair(S.data() + 45 * (size_t)p, norm.data() + TV_NORM * (size_t)p, Fm.data() + 9 * (size_t)p, &ratio[p]);
      if (st[p])
        for (int j = 0; j < 9; ++j) Fm[9 * (size_t)p + j] = NAN;
    }
    MVBA_HIP(hipMemcpy(dF, Fm.data(), sizeof(double) * 9 * np, hipMemcpyHostToDevice));
    ev.mark();
    for (int p0 = 0; p0 < np; p0 += tile) {
      const int cnt = std::min(tile, np - p0);
      hipLaunchKernelGGL(k_twoview_chunk<3>, dim3((unsigned)n_ch, (unsigned)cnt), dim3(START_CHUNK), 0, 0, (long long)n_points, n_images, dptr, dcam, dxy,
                         dpairs + 2 * (size_t)p0, dF + 9 * (size_t)p0, dpart);
      combine(cnt, 1, dS + (size_t)p0, 1);
    }
    ev.mark();
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(Sr.data(), dS, sizeof(double) * np, hipMemcpyDeviceToHost));
    if (timings_ms) {
      timings_ms[1] = ev.ms(0, 1) + ev.ms(2, 3);
      timings_ms[2] = lap_rest(clk.lap(), timings_ms[1]);  // the copies back, the host's eigen-solves and the upload of F
    }
  }
  for (int p = 0; p < np; ++p) {
    const double n = norm[TV_NORM * (size_t)p + 6];
    for (int j = 0; j < 9; ++j) F[9 * (size_t)p + j] = Fm[9 * (size_t)p + j];
    if (n_shared) n_shared[p] = (int64_t)n;
    if (status) status[p] = st[p];
    if (quality) {
      quality[2 * p] = st[p] == 0 ? sqrt(Sr[p] / n) : NAN;
      quality[2 * p + 1] = st[p] == 0 ? ratio[p] : NAN;
    }
  }
  return MVBA_OK;
}

}  // extern "C"
