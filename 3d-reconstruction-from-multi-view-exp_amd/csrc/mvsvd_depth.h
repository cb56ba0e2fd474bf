// The projective-depth iteration (mvsvd_depth_step) -- kernels, gfx950: the arithmetic of one observation that every form of the
// update shares (primary_companion_add, primary_xi, dual_xi, reproj_err2, dominant_eigvec4, fast_rsqrt / fast_rcp) and the kernels
// that read S from memory: the route that factorises the re-weighted matrix first (more than FZ_MAXM images or an odd count, fp32,
// MVSVD_DEPTH_UNFUSED).  Included by mvsvd.hip inside its device-code namespace, after mvsvd_jacobi.h (jacobi_rotation) and
// mvsvd_rows.h (tile_load / tile_store, RowLanes, wave_strided_sum, block_sum_to).  Reached from mvsvd_depth_step through depth_step
// in mvsvd.hip; k_depth_error also ends the fused route's step.

// ---- projective-depth iteration on the device (mvsvd_depth_step; ref lib/perspective_camera_calibration.py:93-129
// primary, :182-224 dual).  After the factorisation of the re-weighted matrix the workspace holds M = U[:, :4]
// (dMr, [3m][4]) and S = diag(sigma) Vt[:4] (dS, [4][rows]); the depth update reads them, the resident observations
// X ([rows][3m]) and writes the new depths z ([rows][m]) -- nothing crosses PCIe but the reprojection error.
// The eigenproblems in their low-rank form (oracle/depth_oracle.py restates them in NumPy):
//   primary  per point a: C[k][i] = (x_ak . u_ki) / |x_ak| (m x 4); dominant eigenvector v of the 4 x 4 companion
//            C^T C by cyclic Jacobi in registers; xi = C v / |C v|  (= the dominant eigenvector of the reference's
//            m x m matrix C C^T, :99-118)
//   dual     per image k: Z[a] = V4[a] (x) x_ak / |x_ak| (rows x 12), V4 = right singular vectors; the 12 x 12
//            companion Z^T Z = sum_a (v v^T) (x) (x^ x^^T) has 10 x 6 distinct entries, summed over the rows per block
//            in row order and over the blocks in block order (no atomics); batched Jacobi; xi = Z w / sqrt(lambda)
//            (= the dominant eigenvector of the reference's N x N matrix, :188-213, in O(N) memory)
// Signs: xi of a point is flipped when its sum is negative (ref :121 / :217); in the dual form every image's vector is
// first oriented to a non-negative sum (the reference inherits LAPACK's eigenvector sign there: projectively equivalent).
// Reprojection error (:43-58) from the same M, S, per-thread sums in row order, fixed tree, fixed block order.

// 1 / sqrt(u) and 1 / u from the hardware seeds and two Newton steps each (full double precision to an ulp or two): the
// per-point kernels below take a root and up to four quotients per observation, and the library sqrt / divide expansions
// (~35 instructions each) were most of their 1.5 ms at 5 M points x 8 images
__device__ __forceinline__ double fast_rsqrt(double u) {
  double r = __builtin_amdgcn_rsq(u);
  r = r * fma(-0.5 * u * r, r, 1.5);
  return r * fma(-0.5 * u * r, r, 1.5);
}
__device__ __forceinline__ double fast_rcp(double u) {
  double r = __builtin_amdgcn_rcp(u);
  r = fma(fma(-u, r, 1.0), r, r);
  return fma(fma(-u, r, 1.0), r, r);
}

// dominant eigenvector of the symmetric 4 x 4 matrix g (upper triangle, row-major 10 values): cyclic Jacobi with
// the rotations of the small solver above (same (c, s) convention), everything in registers
__device__ __forceinline__ void dominant_eigvec4(const double (&g)[10], double (&v)[4]) {
  double A[4][4], V[4][4];
  {
    int e = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j, ++e) A[i][j] = A[j][i] = g[e];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  const double tol2 = 1e-30;
  for (int sweep = 0; sweep < 24; ++sweep) {
    bool any = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double c, sn;
        if (!jacobi_rotation(A[p][p], A[p][q], A[q][q], tol2, c, sn)) continue;
        any = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // rows p, q
          const double ap = A[p][j], aq = A[q][j];
          A[p][j] = c * ap - sn * aq;
          A[q][j] = sn * ap + c * aq;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // columns p, q (and the eigenvectors)
          const double ap = A[i][p], aq = A[i][q];
          A[i][p] = c * ap - sn * aq;
          A[i][q] = sn * ap + c * aq;
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - sn * vq;
          V[i][q] = sn * vp + c * vq;
        }
        const double sym = 0.5 * (A[p][q] + A[q][p]);  // (annihilated up to rounding; keep the two copies equal)
        A[p][q] = A[q][p] = sym;
      }
    if (!any) break;
  }
  // (the largest diagonal entry tracked in a scalar: `A[best][best]` with a run-time `best` put the whole of A into scratch
  // memory -- 144 bytes per lane, stored and reloaded around every rotation of the loop above)
  int best = 0;
  double bestv = A[0][0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (A[i][i] > bestv) { best = i; bestv = A[i][i]; }
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = best == 0 ? V[i][0] : (best == 1 ? V[i][1] : (best == 2 ? V[i][2] : V[i][3]));
}

// squared reprojection error of observation x (3) under P = U4_k (3 x 4) and the point's S column
__device__ __forceinline__ double reproj_err2(const double *u /*[3][4]*/, const double (&s)[4], double x0, double x1, double x2) {
  const double p0 = u[0] * s[0] + u[1] * s[1] + u[2] * s[2] + u[3] * s[3];
  const double p1 = u[4] * s[0] + u[5] * s[1] + u[6] * s[2] + u[7] * s[3];
  const double p2 = u[8] * s[0] + u[9] * s[1] + u[10] * s[2] + u[11] * s[3];
  const double rp = fast_rcp(p2);
  const double d0 = x0 - p0 * rp, d1 = x1 - p1 * rp, d2 = x2 - p2 * rp;
  return d0 * d0 + d1 * d1 + d2 * d2;
}

// ---- one observation x_ak = (x0, x1, x2), inv = 1 / |x_ak|, in the two updates; u = U4_k [3][4], w = w_k [4][3].  Written once
// for the three geometries of each update (a lane per point through LDS tiles, the lanes across a point's images, the fused route;
// k_dual_apply_wide alone keeps its own copy of the dual xi, see there).
// Primary, first pass: d[i] = x . U_k[:, i] (handed back: k_primary_xz forms S from the same products), C[k][i] = d[i] / |x|, and
// the 4 x 4 companion C^T C (upper triangle, row-major) takes its share
__device__ __forceinline__ void primary_companion_add(const double *u, double x0, double x1, double x2, double inv, double (&g)[10], double (&d)[4]) {
  double c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    d[i] = x0 * u[i] + x1 * u[4 + i] + x2 * u[8 + i];
    c[i] = d[i] * inv;
  }
  int e = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j, ++e) g[e] = fma(c[i], c[j], g[e]);
}
// primary, second pass: xi_k = C[k] . v (unnormalised), v the companion's dominant eigenvector
__device__ __forceinline__ double primary_xi(const double *u, double x0, double x1, double x2, double inv, const double (&v)[4]) {
  double xi = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) xi = fma((x0 * u[i] + x1 * u[4 + i] + x2 * u[8 + i]) * inv, v[i], xi);
  return xi;
}
// dual, last pass: xi[a][k] = Z_k[a] . w_k with Z_k[a] = v4 (x) x^, x^ = x / |x| the normalised observation
__device__ __forceinline__ double dual_xi(const double (&v4)[4], double x0, double x1, double x2, double inv, const double *w) {
  const double h0 = x0 * inv, h1 = x1 * inv, h2 = x2 * inv;
  double xi = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) xi = fma(v4[i], h0 * w[3 * i] + h1 * w[3 * i + 1] + h2 * w[3 * i + 2], xi);
  return xi;
}

// primary update, a lane per point: a wave's 64 rows of X go through an LDS tile, the new depths leave through it
template <typename T>
__global__ __launch_bounds__(256) void k_depth_primary(const T *__restrict__ X, const double *__restrict__ Mr, const T *__restrict__ S,
                                                       long long n_rows, int m, T *__restrict__ z, double *__restrict__ Epart) {
  extern __shared__ double sU[];  // [3m][4], then one tile of 64 x [3m values | m depths] per wave
  for (int q = threadIdx.x; q < 12 * m; q += blockDim.x) sU[q] = Mr[q];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = 3 * m, ldt = (n + m) | 1;
  T *tile = reinterpret_cast<T *>(sU + 12 * (size_t)m) + (size_t)wave * 64 * ldt;
  double esum = 0.0;
  for (long long base = ((long long)blockIdx.x * 4 + wave) * 64; base < n_rows; base += (long long)gridDim.x * 256) {
    const int rows_here = (int)min<long long>(64, n_rows - base);
    tile_load(X, base, rows_here, n, tile, ldt, lane);
    wave_sync();
    if (lane < rows_here) {
      const long long a = base + lane;
      const T *xr = tile + lane * ldt;
      T *zr = tile + lane * ldt + n;
      double s[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = (double)S[(size_t)i * n_rows + a];
      double g[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, d[4];
      for (int k = 0; k < m; ++k) {
        const double x0 = (double)xr[3 * k], x1 = (double)xr[3 * k + 1], x2 = (double)xr[3 * k + 2];
        const double *u = sU + 12 * k;
        primary_companion_add(u, x0, x1, x2, fast_rsqrt(x0 * x0 + x1 * x1 + x2 * x2), g, d);
        esum += reproj_err2(u, s, x0, x1, x2);
      }
      double v[4];
      dominant_eigvec4(g, v);
      double nrm2 = 0.0, sum = 0.0;
      for (int k = 0; k < m; ++k) {  // z <- xi_k / |x_ak| for now
        const double x0 = (double)xr[3 * k], x1 = (double)xr[3 * k + 1], x2 = (double)xr[3 * k + 2];
        const double inv = fast_rsqrt(x0 * x0 + x1 * x1 + x2 * x2);
        const double xi = primary_xi(sU + 12 * k, x0, x1, x2, inv, v);
        nrm2 = fma(xi, xi, nrm2);
        sum += xi;
        zr[k] = (T)(xi * inv);
      }
      const double sc = (sum < 0.0 ? -1.0 : 1.0) * fast_rsqrt(nrm2);  // unit length, non-negative sum (ref :118, :121)
      for (int k = 0; k < m; ++k) zr[k] = (T)((double)zr[k] * sc);
    }
    wave_sync();
    tile_store(z, base, rows_here, m, tile + n, ldt, lane);
    wave_sync();
  }
  block_sum_to(esum, Epart);
}

// Rows too long for the LDS tiles (fp64 from ~15 images on): the lanes of a wave run ACROSS the images of a point -- P = m rounded
// up to a power of two (at most 64) lanes per point, 64 / P points per pass -- so that a pass reads one contiguous range of X
// and writes one of z; the sums over a point's images (the 4 x 4 companion, the norm and the sign of the new depths) are fixed
// trees over its lanes, and every lane of a point finds the companion's eigenvector itself.  (The lane-per-point form walks
// 24 m bytes of its own row per lane: 1.6 ms at 1 M points x 30 images against 0.4 for this one.)
template <typename T>
__global__ __launch_bounds__(256) void k_depth_primary_wide(const T *__restrict__ X, const double *__restrict__ Mr, const T *__restrict__ S,
                                                            long long n_rows, int m, T *__restrict__ z, double *__restrict__ Epart) {
  extern __shared__ double sU[];  // [m][3][4], then per wave [64 points][10 companion sums | 4 eigenvector components]
  for (int q = threadIdx.x; q < 12 * m; q += blockDim.x) sU[q] = Mr[q];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = 3 * m;
  double *sg = sU + 12 * (size_t)m + (size_t)wv * 64 * 14;
  const RowLanes L(m, lane);
  const long long wave = (long long)blockIdx.x * 4 + wv, n_waves = (long long)gridDim.x * 4;
  double esum = 0.0;
  // a batch = 64 points: (1) their companions, R points per pass, the lanes across the images; (2) the 64 eigenvectors, a lane per
  // point (the 4 x 4 Jacobi is ~1000 instructions: run once per pass of R points it was most of the kernel); (3) the new depths
  for (long long b0 = wave * 64; b0 < n_rows; b0 += n_waves * 64) {
    for (int sub = 0; sub < 64; sub += L.R) {
      const long long a = min(b0 + sub + L.rr, n_rows - 1);  // (a clamped row repeats the last one: computed, never stored)
      const bool row_ok = b0 + sub + L.rr < n_rows;
      const T *xr = X + a * n;
      double s[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = (double)S[(size_t)i * n_rows + a];
      double g[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, d[4];
      for (int k = L.g0; k < m; k += L.P) {
        const double x0 = (double)xr[3 * k], x1 = (double)xr[3 * k + 1], x2 = (double)xr[3 * k + 2];
        const double *u = sU + 12 * k;
        primary_companion_add(u, x0, x1, x2, fast_rsqrt(x0 * x0 + x1 * x1 + x2 * x2), g, d);
        if (row_ok) esum += reproj_err2(u, s, x0, x1, x2);
      }
#pragma unroll
      for (int e = 0; e < 10; ++e) {
        L.sum(g[e]);
        if (L.g0 == 0) sg[(sub + L.rr) * 14 + e] = g[e];
      }
    }
    wave_sync();
    {
      double g[10], v[4];
#pragma unroll
      for (int e = 0; e < 10; ++e) g[e] = sg[lane * 14 + e];
      dominant_eigvec4(g, v);
#pragma unroll
      for (int i = 0; i < 4; ++i) sg[lane * 14 + 10 + i] = v[i];
    }
    wave_sync();
    for (int sub = 0; sub < 64; sub += L.R) {
      const long long a = min(b0 + sub + L.rr, n_rows - 1);
      const bool row_ok = b0 + sub + L.rr < n_rows;
      const T *xr = X + a * n;
      double v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = sg[(sub + L.rr) * 14 + 10 + i];
      double nrm2 = 0.0, sum = 0.0;
      for (int k = L.g0; k < m; k += L.P) {
        const double x0 = (double)xr[3 * k], x1 = (double)xr[3 * k + 1], x2 = (double)xr[3 * k + 2];
        const double inv = fast_rsqrt(x0 * x0 + x1 * x1 + x2 * x2);
        const double xi = primary_xi(sU + 12 * k, x0, x1, x2, inv, v);
        nrm2 = fma(xi, xi, nrm2);
        sum += xi;
        if (row_ok) z[a * m + k] = (T)(xi * inv);
      }
      L.sum(nrm2, sum);
      const double sc = (sum < 0.0 ? -1.0 : 1.0) * fast_rsqrt(nrm2);  // unit length, non-negative sum (ref :118, :121)
      if (row_ok)
        for (int k = L.g0; k < m; k += L.P) z[a * m + k] = (T)((double)z[a * m + k] * sc);  // (this lane's own stores)
    }
    wave_sync();
  }
  block_sum_to(esum, Epart);
}

// the dual update's last pass in the same geometry: xi[a][k] = Z_k[a] . w_k, the point's sign rule, z = xi / |x|, reprojection error
template <typename T>
__global__ __launch_bounds__(256) void k_dual_apply_wide(const T *__restrict__ X, const T *__restrict__ S, double is0, double is1, double is2,
                                                         double is3, const double *__restrict__ Mr, const double *__restrict__ w12,
                                                         long long n_rows, int m, T *__restrict__ z, double *__restrict__ Epart) {
  extern __shared__ double sm[];  // U4 [m][3][4], w [m][12]
  double *sU = sm, *sW = sm + 12 * (size_t)m;
  for (int q = threadIdx.x; q < 12 * m; q += blockDim.x) { sU[q] = Mr[q]; sW[q] = w12[q]; }
  __syncthreads();
  const int n = 3 * m;
  const RowLanes L(m, threadIdx.x & 63);
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * 4;
  double esum = 0.0;
  for (long long a0 = wave * L.R; a0 < n_rows; a0 += n_waves * L.R) {
    const long long a = min(a0 + L.rr, n_rows - 1);
    const bool row_ok = a0 + L.rr < n_rows;
    const T *xr = X + a * n;
    double s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = (double)S[(size_t)i * n_rows + a];
    const double v4[4] = {s[0] * is0, s[1] * is1, s[2] * is2, s[3] * is3};
    double sum = 0.0;
    for (int k = L.g0; k < m; k += L.P) {
      const double x0 = (double)xr[3 * k], x1 = (double)xr[3 * k + 1], x2 = (double)xr[3 * k + 2];
      const double inv = fast_rsqrt(x0 * x0 + x1 * x1 + x2 * x2);
      const double h0 = x0 * inv, h1 = x1 * inv, h2 = x2 * inv;
      const double *w = sW + 12 * k;
      double xi = 0.0;  // (dual_xi's arithmetic, written out: through the helper the float form took 72 registers instead of 64, seven waves per SIMD instead of eight)
#pragma unroll
      for (int i = 0; i < 4; ++i) xi = fma(v4[i], h0 * w[3 * i] + h1 * w[3 * i + 1] + h2 * w[3 * i + 2], xi);
      sum += xi;
      if (row_ok) {
        z[a * m + k] = (T)(xi * inv);
        esum += reproj_err2(sU + 12 * k, s, x0, x1, x2);
      }
    }
    L.sum(sum);
    if (sum < 0.0 && row_ok)
      for (int k = L.g0; k < m; k += L.P) z[a * m + k] = (T)(-(double)z[a * m + k]);  // ref :217
  }
  block_sum_to(esum, Epart);
}

// dual, pass 1: per block and image the 60 distinct entries of sum_a (v v^T) (x) (x^ x^^T) and the 12 column sums of Z, laid out
// as 14 "tasks" of 6 values per image for k_dual_reduce: task t < 10 m = image t / 10, pair (i <= j) of V4 components t % 10 -> the 6
// sums over (c <= d); task 10 m <= t < 14 m = image, component i -> 3 column sums.
// A thread owns ONE image (all 72 sums of it in registers) and the rows rr = sub, sub + nsplit, ... of the staged batch, with
// nsplit = 256 / min(m, 256) thread groups per block and a partial per group (summed in group order by k_dual_reduce); more than
// 256 images go in chunks of 256, the rows staged again per chunk.  Per row a thread reads its image's normalised observation
// (3 values) and the row's v4 (4, broadcast) for 82 multiply-adds -- rounds 4-5 had a thread per TASK reading five values for
// seven multiply-adds, and the kernel ran at the LDS read rate: 1.76 ms at 1 M points x 30 images, this form 0.5.
__constant__ int c_pair_i[10] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3};
__constant__ int c_pair_j[10] = {0, 1, 2, 3, 1, 2, 3, 2, 3, 3};
inline int dual_gram_split(int m) { return std::min(16, 256 / std::min(m, 256)); }  // thread groups (= partials) per block
template <typename T>
__global__ __launch_bounds__(256) void k_dual_gram(const T *__restrict__ X, const T *__restrict__ S, double is0, double is1, double is2,
                                                   double is3, long long n_rows, int m, long long rows_per_block, int DG_ROWS,
                                                   double *__restrict__ part /*[blocks][nsplit][14 m][6]*/) {
  // staged per pass: x^ [DG_ROWS][3m] (stride 3m | 1) and v4 [DG_ROWS][4]: the normalisation happens once per (row, image)
  extern __shared__ double sg[];
  const int n = 3 * m, ldx = n | 1;
  double *sx = sg, *sv = sg + (size_t)DG_ROWS * ldx;
  const long long a0 = (long long)blockIdx.x * rows_per_block, a1 = min(n_rows, a0 + rows_per_block);
  const double isg[4] = {is0, is1, is2, is3};
  const int tpi = min(m, 256), nsplit = min(16, 256 / tpi), sub = (int)threadIdx.x / tpi, kl = (int)threadIdx.x - sub * tpi;
  for (int k0 = 0; k0 < m; k0 += tpi) {
    const int k = k0 + kl;
    const bool mine = sub < nsplit && k < m;
    double acc[10][6], col[4][3];
#pragma unroll
    for (int p = 0; p < 10; ++p)
#pragma unroll
      for (int q = 0; q < 6; ++q) acc[p][q] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) col[i][c] = 0.0;
    for (long long r0 = a0; r0 < a1; r0 += DG_ROWS) {
      const int nr = (int)min<long long>(DG_ROWS, a1 - r0);
      __syncthreads();
      for (int e = threadIdx.x; e < nr * m; e += 256) {  // (row, image): normalise
        const int rr = e / m, kk = e - rr * m;
        const T *xr = X + (r0 + rr) * n + 3 * kk;
        const double x0 = (double)xr[0], x1 = (double)xr[1], x2 = (double)xr[2];
        const double inv = fast_rsqrt(x0 * x0 + x1 * x1 + x2 * x2);
        double *d = sx + (size_t)rr * ldx + 3 * kk;
        d[0] = x0 * inv; d[1] = x1 * inv; d[2] = x2 * inv;
      }
      for (int e = threadIdx.x; e < nr * 4; e += 256) sv[e] = (double)S[(size_t)(e & 3) * n_rows + r0 + (e >> 2)] * isg[e & 3];
      __syncthreads();
      if (mine)
        for (int rr = sub; rr < nr; rr += nsplit) {
          const double *hp = sx + (size_t)rr * ldx + 3 * k;
          const double h[3] = {hp[0], hp[1], hp[2]};
          const double v[4] = {sv[4 * rr], sv[4 * rr + 1], sv[4 * rr + 2], sv[4 * rr + 3]};
          const double hh[6] = {h[0] * h[0], h[0] * h[1], h[0] * h[2], h[1] * h[1], h[1] * h[2], h[2] * h[2]};
          int p = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) col[i][c] = fma(v[i], h[c], col[i][c]);
#pragma unroll
            for (int j = i; j < 4; ++j, ++p) {
              const double pq = v[i] * v[j];
#pragma unroll
              for (int q = 0; q < 6; ++q) acc[p][q] = fma(pq, hh[q], acc[p][q]);
            }
          }
        }
    }
    if (mine) {
      double *o = part + (size_t)(blockIdx.x * nsplit + sub) * 14 * m * 6;
#pragma unroll
      for (int p = 0; p < 10; ++p)
#pragma unroll
        for (int q = 0; q < 6; ++q) o[((size_t)10 * k + p) * 6 + q] = acc[p][q];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[((size_t)10 * m + 4 * k + i) * 6 + c] = col[i][c];
#pragma unroll
        for (int c = 3; c < 6; ++c) o[((size_t)10 * m + 4 * k + i) * 6 + c] = 0.0;
      }
    }
  }
}

// dual, pass 2: block partials summed in block order -> G12[k][12][12] (symmetric, index (i, c) = 3 i + c) and colsum[k][12]
__global__ void k_dual_reduce(const double *__restrict__ part, int blocks, int m, double *__restrict__ G12, double *__restrict__ colsum) {
  const int t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;  // one wave per sum
  if (t >= 14 * m * 6) return;
  const int task = t / 6, q = t % 6;
  const double v = wave_strided_sum(part + (size_t)task * 6 + q, blocks, (size_t)14 * m * 6, lane);
  if (lane) return;
  if (task < 10 * m) {
    const int k = task / 10, i = c_pair_i[task % 10], j = c_pair_j[task % 10];
    const int c = q < 3 ? 0 : (q < 5 ? 1 : 2), d = q < 3 ? q : (q < 5 ? q - 2 : 2);
    double *G = G12 + (size_t)k * 144;
    G[(3 * i + c) * 12 + 3 * j + d] = v; G[(3 * i + d) * 12 + 3 * j + c] = v;
    G[(3 * j + c) * 12 + 3 * i + d] = v; G[(3 * j + d) * 12 + 3 * i + c] = v;
  } else if (q < 3) {
    const int k = (task - 10 * m) / 4, i = (task - 10 * m) % 4;
    colsum[(size_t)k * 12 + 3 * i + q] = v;
  }
}

// dual, pass 3 (after the batched Jacobi: eigenvalues on the diagonal of G12[k], eigenvectors in the columns of V12[k]):
// w_k = +- v_max / sqrt(lambda_max), oriented so that the image's depth vector Z w has a non-negative sum
__global__ void k_dual_vec(const double *__restrict__ G12, const double *__restrict__ V12, const double *__restrict__ colsum, int m,
                           double *__restrict__ w12, int *__restrict__ flag) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const double *G = G12 + (size_t)k * 144, *V = V12 + (size_t)k * 144;
  int best = 0;
  for (int i = 1; i < 12; ++i)
    if (G[i * 13] > G[best * 13]) best = i;
  const double lam = G[best * 13];
  if (!(lam > 0.0)) { atomicOr(flag, 1); return; }
  double dot = 0.0;
  for (int i = 0; i < 12; ++i) dot += colsum[(size_t)k * 12 + i] * V[i * 12 + best];
  const double sc = (dot < 0.0 ? -1.0 : 1.0) / sqrt(lam);
  for (int i = 0; i < 12; ++i) w12[(size_t)k * 12 + i] = sc * V[i * 12 + best];
}

// dual, pass 4, a lane per point through LDS tiles: xi[a][k] = Z_k[a] . w_k, the row's sign rule, z = xi / |x|, reprojection error
template <typename T>
__global__ __launch_bounds__(256) void k_dual_apply(const T *__restrict__ X, const T *__restrict__ S, double is0, double is1, double is2,
                                                    double is3, const double *__restrict__ Mr, const double *__restrict__ w12,
                                                    long long n_rows, int m, T *__restrict__ z, double *__restrict__ Epart) {
  extern __shared__ double sm[];  // U4 [3m][4], w [m][12], then one tile of 64 x [3m values | m depths] per wave
  double *sU = sm, *sW = sm + 12 * (size_t)m;
  for (int q = threadIdx.x; q < 12 * m; q += blockDim.x) { sU[q] = Mr[q]; sW[q] = w12[q]; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = 3 * m, ldt = (n + m) | 1;
  T *tile = reinterpret_cast<T *>(sm + 24 * (size_t)m) + (size_t)wave * 64 * ldt;
  double esum = 0.0;
  for (long long base = ((long long)blockIdx.x * 4 + wave) * 64; base < n_rows; base += (long long)gridDim.x * 256) {
    const int rows_here = (int)min<long long>(64, n_rows - base);
    tile_load(X, base, rows_here, n, tile, ldt, lane);
    wave_sync();
    if (lane < rows_here) {
      const long long a = base + lane;
      const T *xr = tile + lane * ldt;
      T *zr = tile + lane * ldt + n;
      double s[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = (double)S[(size_t)i * n_rows + a];
      const double v4[4] = {s[0] * is0, s[1] * is1, s[2] * is2, s[3] * is3};
      double sum = 0.0;
      for (int k = 0; k < m; ++k) {
        const double x0 = (double)xr[3 * k], x1 = (double)xr[3 * k + 1], x2 = (double)xr[3 * k + 2];
        const double inv = fast_rsqrt(x0 * x0 + x1 * x1 + x2 * x2);
        const double xi = dual_xi(v4, x0, x1, x2, inv, sW + 12 * k);
        sum += xi;
        zr[k] = (T)(xi * inv);
        esum += reproj_err2(sU + 12 * k, s, x0, x1, x2);
      }
      if (sum < 0.0)
        for (int k = 0; k < m; ++k) zr[k] = (T)(-(double)zr[k]);  // ref :217
    }
    wave_sync();
    tile_store(z, base, rows_here, m, tile + n, ldt, lane);
    wave_sync();
  }
  block_sum_to(esum, Epart);
}

__global__ void k_depth_error(const double *__restrict__ Epart, int blocks, double count, double f0, double *__restrict__ out) {
  const double t = wave_strided_sum(Epart, blocks, 1, (int)threadIdx.x);  // one wave
  if (threadIdx.x == 0) out[0] = f0 * sqrt(t / count);  // ref :56
}
