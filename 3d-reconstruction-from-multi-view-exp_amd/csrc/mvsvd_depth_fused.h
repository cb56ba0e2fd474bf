// The projective-depth iteration that never writes the re-weighted matrix (mvsvd_depth_step, fp64, an even image count up to
// FZ_MAXM; round 5) -- kernels, gfx950: the double2 row staging, the Gram passes of X o z, the depth updates with S formed on the fly.
// Included by mvsvd.hip inside its device-code namespace, last of the mvsvd_*.h headers: uses gram_store_partial and tile_elem
// (mvsvd_gram.h), tile_load / tile_store, wave_strided_sum and block_sum_to (mvsvd_rows.h) and the shared depth arithmetic
// (mvsvd_depth.h).  Reached from mvsvd_depth_step through depth_step_fused in mvsvd.hip (launch_gram_xz and the kernel tables).
//
// Round 4's iteration made ~7 passes over a 0.96 GB matrix at 5 M points x 8 images (write W = X o z normalised, Gram, rotate W V1
// into B, Gram of B, project S = M^T W, update) for ~1.5 GB of unavoidable traffic.  For few images (n = 3 m <= 32 columns, n even:
// the domain of the LDS-staged Gram kernel) nothing but X and z is streamed any more:
//   k_gram_xz<M, NORM, false>  Gram of W formed on the fly: a workgroup stages 128 rows of X and of z, scales the rows IN LDS (norm 1:
//                 every row to unit length; norm 2: every image by its global scale cs), then the MFMA loop of k_gram_fused
//   k_gram_xz<M, NORM, true>   the refinement pass in one kernel: the same staging, B = W V1 on the matrix cores into a second LDS
//                 tile, Gram of B from there -- B never exists in memory
//   k_primary_xz / k_dual_gram_mfma / k_dual_apply_xz   the depth updates with S = M^T W formed per row from X, z and M (24 x 4
//                 products) instead of read from a projection pass; the dual update also leaves the per-image sums of (x z)^2 of
//                 the NEW depths behind (the next iteration's norm-2 scales), so k_group_sumsq runs once per loop, not once per step
// Same arithmetic per entry as before up to the order of a few sums; oracle parity per step stays at 1e-9 (tests).

// Whole rows on their way into LDS as pairs of doubles held in registers: thread t of `stride` takes the pairs t, t + stride, ...
// of the nv that start at element e0 of src (e0 even, src 16-byte aligned).  A pair that reaches past `total`, the end of src,
// comes element by element with a zero for what is missing; slots past nv are zeros and are not stored.
template <int NV>
__device__ __forceinline__ void stage_load(const double *__restrict__ src, long long e0, long long total, int nv, int t, int stride, double2 (&r)[NV]) {
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int v = t + stride * u;
    const long long i = e0 + 2LL * v;
    if (v < nv && i + 2 <= total) r[u] = *reinterpret_cast<const double2 *>(src + i);
    else r[u] = double2{(v < nv && i < total) ? src[i] : 0.0, 0.0};
  }
}
template <int NV>
__device__ __forceinline__ void stage_store(const double2 (&r)[NV], int nv, int t, int stride, double *dst) {
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int v = t + stride * u;
    if (v < nv) *reinterpret_cast<double2 *>(dst + 2 * v) = r[u];
  }
}

// Stage GRAM_ROWS rows of X ([rows][n]) and z ([rows][m]) and scale them in place: sx[r][c] <- x z[r][c / 3] s.
// NORM 1: s = 1 / |row of X o z|; NORM 2: s = cs[c / 3].  Rows past the end become zeros.  sp: [GRAM_ROWS][m] scratch.
struct FzRegs {
  double2 xs[GRAM_ROWS * 32 / 2 / 256];
  double2 zs[(GRAM_ROWS * FZ_MAXM / 2 + 255) / 256];
};
__device__ __forceinline__ void fz_load(const double *__restrict__ X, const double *__restrict__ z, long long r0, long long n_rows, int n, int m, FzRegs &R) {
  stage_load(X, r0 * n, n_rows * n, GRAM_ROWS * n / 2, threadIdx.x, 256, R.xs);  // (r0 is a multiple of 128: both offsets 16-byte aligned)
  stage_load(z, r0 * m, n_rows * m, GRAM_ROWS * m / 2, threadIdx.x, 256, R.zs);
}
template <int NORM>
__device__ __forceinline__ void fz_stage(const FzRegs &R, long long r0, long long n_rows, int n, int m, const double *__restrict__ cs,
                                         double *sx, double *sz, double *sp) {
  stage_store(R.xs, GRAM_ROWS * n / 2, threadIdx.x, 256, sx);
  stage_store(R.zs, GRAM_ROWS * m / 2, threadIdx.x, 256, sz);
  __syncthreads();
  if (NORM == 1) {  // per (row, image): z^2 |x|^2; then ONE reciprocal root per row (the full-precision divide and root per
    // (row, image) of the first build cost 0.1 ms per pass at 5 M x 8); then the scaling
    for (int e = threadIdx.x; e < GRAM_ROWS * m; e += 256) {
      const int r = e / m, g = e - r * m;
      const double *x = sx + r * n + 3 * g;
      const double zz = sz[e];
      sp[e] = zz * zz * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    }
    __syncthreads();
    if (threadIdx.x < GRAM_ROWS) {
      const int r = threadIdx.x;
      double ss = 0.0;
      for (int q = 0; q < m; ++q) ss += sp[r * m + q];
      sp[r * m] = (r0 + r < n_rows) ? fast_rsqrt(ss) : 0.0;  // (the row's slot 0: its partials have been read by this thread alone)
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < GRAM_ROWS * m; e += 256) {
    const int r = e / m, g = e - r * m;
    const double f = NORM == 1 ? sz[e] * sp[r * m] : sz[e] * cs[g];
    double *x = sx + r * n + 3 * g;
    x[0] *= f; x[1] *= f; x[2] *= f;
  }
  __syncthreads();
}

// the MFMA loop of k_gram_fused over the wave's 32 staged rows (`rows` = this lane's first row in a row-major [.][n] tile)
template <int MODE>
__device__ __forceinline__ void fz_gram_rows(const double *rows, int n, const int *col, const bool *cok, svd_d4 *acc) {
  constexpr int NC = MODE == 1 ? 1 : (MODE == 2 ? 3 : 2);
#pragma unroll
  for (int g = 0; g < ROWS_PER_STEP / 4; ++g) {
    double v[NC];
#pragma unroll
    for (int t = 0; t < NC; ++t) v[t] = cok[t] ? rows[(4 * g) * n + col[t]] : 0.0;
    if (MODE == 2) {
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[0], v[0], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[1], v[2], acc[1], 0, 0, 0);
    } else {
      int q = 0;
#pragma unroll
      for (int t = 0; t < NC; ++t)
#pragma unroll
        for (int u = t; u < NC; ++u, ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[t], v[u], acc[q], 0, 0, 0);
    }
  }
}

// ROT: the refinement pass (B = W V1 on the matrix cores into a second tile, Gram of B); else the first pass (Gram of W)
template <int M, int NORM, bool ROT>  // M images at compile time (the staging's divisions by m become shifts and multiplies)
__global__ __launch_bounds__(256) void k_gram_xz(const double *__restrict__ X, const double *__restrict__ z, long long n_rows, int n_rt, int m_rt,
                                                 const double *__restrict__ cs, const double *__restrict__ V1, double *__restrict__ partial) {
  constexpr int m = M, n = 3 * M, MODE = n <= 16 ? 1 : (n <= 24 ? 2 : 3);
  (void)n_rt; (void)m_rt;
  extern __shared__ double fz_lds[];
  double *sx = fz_lds, *sz = sx + GRAM_ROWS * n, *sp = sz + GRAM_ROWS * m, *sb = sp + GRAM_ROWS * m;  // sb only when ROT
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  constexpr int NP = MODE == 1 ? 1 : (MODE == 2 ? 2 : 3);
  constexpr int NC = MODE == 1 ? 1 : (MODE == 2 ? 3 : 2);
  svd_d4 acc[3] = {svd_d4{0, 0, 0, 0}, svd_d4{0, 0, 0, 0}, svd_d4{0, 0, 0, 0}};
  int col[NC];
  bool cok[NC];
#pragma unroll
  for (int t = 0; t < NC; ++t) {
    const int c = MODE == 2 ? (t == 0 ? li : (t == 1 ? 8 + li : (li < 8 ? 16 + li : li - 8))) : GT * t + li;
    cok[t] = c < n; col[t] = min(c, n - 1);
  }
  const int nct = (n + 15) / 16, ng = (n + 3) / 4;
  double vb[2][8];
  if (ROT) {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const int k = 4 * g + lk;
#pragma unroll
      for (int c = 0; c < 2; ++c) vb[c][g] = (k < n && 16 * c + li < n) ? V1[(size_t)k * n + 16 * c + li] : 0.0;
    }
  }
  FzRegs R;
  const long long r_first = (long long)blockIdx.y * GRAM_ROWS, r_stride = (long long)gridDim.y * GRAM_ROWS;
  if (r_first < n_rows) fz_load(X, z, r_first, n_rows, n, m, R);
  for (long long r0 = r_first; r0 < n_rows; r0 += r_stride) {
    fz_stage<NORM>(R, r0, n_rows, n, m, cs, sx, sz, sp);
    if (r0 + r_stride < n_rows) fz_load(X, z, r0 + r_stride, n_rows, n, m, R);  // the next step's rows travel under this step's products
    if (ROT) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {  // the wave's two 16-row tiles: B = W V1 (as k_rotate_rows), into the wave's own rows of sb
        const double *rows = sx + (size_t)(wave * ROWS_PER_STEP + 16 * t + li) * n;
        svd_d4 ra[2] = {svd_d4{0, 0, 0, 0}, svd_d4{0, 0, 0, 0}};
#pragma unroll
        for (int g = 0; g < 8; ++g) {
          if (g >= ng) break;
          const int k = 4 * g + lk;
          const double a = (k < n) ? rows[k] : 0.0;
          ra[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, vb[0][g], ra[0], 0, 0, 0);
          if (nct > 1) ra[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, vb[1][g], ra[1], 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // C/D layout: col = li, row = lk + 4 q
          double *orow = sb + (size_t)(wave * ROWS_PER_STEP + 16 * t + lk + 4 * q) * n;
          if (li < n) orow[li] = ra[0][q];
          if (16 + li < n) orow[16 + li] = ra[1][q];
        }
      }
      wave_sync();  // (a wave multiplies the rows of sb it wrote itself)
      fz_gram_rows<MODE>(sb + (size_t)(wave * ROWS_PER_STEP + lk) * n, n, col, cok, acc);
    } else {
      fz_gram_rows<MODE>(sx + (size_t)(wave * ROWS_PER_STEP + lk) * n, n, col, cok, acc);
    }
    __syncthreads();
  }
  gram_store_partial(acc, NP, 0, NP, partial, fz_lds);  // (the staging tile: the last step ended with a barrier; NP x 8 KiB <= 128 n x 8 bytes for n >= 6 ...)
}

// per-point update of the primary scheme (k_depth_primary) with S formed from X, z and M on the fly; z in place
__global__ __launch_bounds__(256, 2) void k_primary_xz(const double *__restrict__ X, const double *__restrict__ Mr, long long n_rows, int m,
                                                    double *__restrict__ z, double *__restrict__ Epart) {
  extern __shared__ double sU[];  // [3m][4], then one tile of 64 x [3m values | m depths] per wave
  for (int q = threadIdx.x; q < 12 * m; q += blockDim.x) sU[q] = Mr[q];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = 3 * m, ldt = (n + m) | 1;
  double *tile = sU + 12 * (size_t)m + (size_t)wave * 64 * ldt;
  double esum = 0.0;
  for (long long base = ((long long)blockIdx.x * 4 + wave) * 64; base < n_rows; base += (long long)gridDim.x * 256) {
    const int rows_here = (int)min<long long>(64, n_rows - base);
    tile_load(X, base, rows_here, n, tile, ldt, lane);
    tile_load(z, base, rows_here, m, tile + n, ldt, lane);
    wave_sync();
    if (lane < rows_here) {
      const double *xr = tile + lane * ldt;
      double *zr = tile + lane * ldt + n;
      double g[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, s[4] = {0, 0, 0, 0}, ss = 0.0;
      for (int k = 0; k < m; ++k) {
        const double x0 = xr[3 * k], x1 = xr[3 * k + 1], x2 = xr[3 * k + 2], zk = zr[k];
        const double n2 = x0 * x0 + x1 * x1 + x2 * x2;
        double d[4];
        primary_companion_add(sU + 12 * k, x0, x1, x2, fast_rsqrt(n2), g, d);
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = fma(zk, d[i], s[i]);  // S = M^T w, w = x z / |row|: the row scale follows below
        ss = fma(zk * zk, n2, ss);
      }
      const double rs = 1.0 / sqrt(ss);
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] *= rs;
      double v[4];
      dominant_eigvec4(g, v);
      double nrm2 = 0.0, sum = 0.0;
      for (int k = 0; k < m; ++k) {
        const double x0 = xr[3 * k], x1 = xr[3 * k + 1], x2 = xr[3 * k + 2];
        const double inv = fast_rsqrt(x0 * x0 + x1 * x1 + x2 * x2);
        const double *u = sU + 12 * k;
        const double xi = primary_xi(u, x0, x1, x2, inv, v);
        esum += reproj_err2(u, s, x0, x1, x2);
        nrm2 = fma(xi, xi, nrm2);
        sum += xi;
        zr[k] = xi * inv;
      }
      const double sc = (sum < 0.0 ? -1.0 : 1.0) * fast_rsqrt(nrm2);
      for (int k = 0; k < m; ++k) zr[k] *= sc;
    }
    wave_sync();
    tile_store(z, base, rows_here, m, tile + n, ldt, lane);
    wave_sync();
  }
  block_sum_to(esum, Epart);
}

// dual scheme, pass 1 with V4 = S diag(1 / sigma) formed from X, z, cs and M while the rows are staged -- and the sums themselves
// on the matrix cores.  (A first build kept k_dual_gram's form, one thread per (image, entry) walking the staged rows: 1.08-1.16 ms at
// 5 M points x 8 images against 0.67 before S moved into the kernel -- the shares of S beside the observations doubled its LDS
// and left two workgroups per CU; 32 rows per pass instead of 128: 0.35 against 0.44 ms at 1 M points.)
// Per image k the 12 x 12 companion is the Gram matrix of Z_k[a] = V4[a] (x) x^_ak
// (rows x 12): one v_mfma_f64_16x16x4_f64 per 4 rows and image with the SAME operand on both sides -- Z_k[row][li], formed per lane
// from the staged V4 and x^ (two LDS reads, one product), column 12 of the 16-wide tile a constant 1 so that row 12 of the result
// is the column sum of Z_k that k_dual_vec needs.  A wave keeps the m tiles of its 32 rows in registers and writes them once:
// part[block x 4 + wave][m][256] in the C/D layout, summed in that order by k_dual_reduce_mfma (no atomics).  One thread per
// (image, entry) walking rows through LDS took 1.08 ms at 5 M points x 8 images (0.67 before S moved into the kernel).
template <int M>  // the image count at compile time (the fused path has m in {2, 4, 6, 8, 10}): no division per staging task, no branch between MFMAs
__global__ __launch_bounds__(256, 2) void k_dual_gram_mfma(const double *__restrict__ X, const double *__restrict__ z, const double *__restrict__ cs,
                                                            const double *__restrict__ Mr, double is0, double is1, double is2, double is3,
                                                            long long n_rows, int m_rt, double *__restrict__ part /*[gridDim.x * 4][m][256]*/) {
  constexpr int m = M;
  (void)m_rt;
  // Every WAVE stages its own 32 rows of a 128-row step (wave-private tiles, no workgroup barrier in the loop): the two waves of a
  // SIMD drift apart and one's staging runs under the other's MFMAs.  (With the workgroup staging 128 rows together behind
  // barriers the waves spent half their time waiting and the matrix cores were 37 % busy: 0.74 ms at 5 M x 8.)
  extern __shared__ double sg[];
  const int n = 3 * m, mp = m | 1, PL = ROWS_PER_STEP * mp + 8;  // shares of S: four planes [row][m | 1]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const int wtile = ROWS_PER_STEP * (n + m + 4) + 4 * PL;        // doubles per wave: x (normalised in place) | z | V4 | shares
  double *sU = sg, *sx = sg + 12 * m + (size_t)wave * wtile, *sz = sx + ROWS_PER_STEP * n, *sv = sz + ROWS_PER_STEP * m, *ssh = sv + 4 * ROWS_PER_STEP;
  for (int q = threadIdx.x; q < 12 * m; q += 256) sU[q] = Mr[q];
  __syncthreads();
  const double isg[4] = {is0, is1, is2, is3};
  const int i3 = min(li / 3, 3), c3 = li - 3 * (li / 3);
  const double one12 = li == 12 ? 1.0 : 0.0, use = li < 12 ? 1.0 : 0.0;
  svd_d4 acc[M];
#pragma unroll
  for (int k = 0; k < M; ++k) acc[k] = svd_d4{0, 0, 0, 0};
  constexpr int MAXX = (ROWS_PER_STEP * 3 * M / 2 + 63) / 64, MAXZ = (ROWS_PER_STEP * M / 2 + 63) / 64;
  double2 xs[MAXX], zs[MAXZ];
  const int nvx = ROWS_PER_STEP * n / 2, nvz = ROWS_PER_STEP * m / 2;
  auto wload = [&](long long rw) {  // this wave's 32 rows from row rw on (a multiple of 32: both offsets 16-byte aligned)
    stage_load(X, rw * n, n_rows * n, nvx, lane, 64, xs);
    stage_load(z, rw * m, n_rows * m, nvz, lane, 64, zs);
  };
  const long long w_first = ((long long)blockIdx.x * 4 + wave) * ROWS_PER_STEP, w_stride = (long long)gridDim.x * 4 * ROWS_PER_STEP;
  if (w_first < n_rows) wload(w_first);
  for (long long rw = w_first; rw < n_rows; rw += w_stride) {
    const int nr = (int)min<long long>(ROWS_PER_STEP, n_rows - rw);
    stage_store(xs, nvx, lane, 64, sx);
    stage_store(zs, nvz, lane, 64, sz);
    wave_sync();
    if (rw + w_stride < n_rows) wload(rw + w_stride);  // the next step's rows travel while this step is staged and multiplied
    for (int e = lane; e < ROWS_PER_STEP * m; e += 64) {  // (row, image): normalise in place; the image's share of S = M^T w
      const int rr = e / m, k = e - rr * m;
      double *d = sx + rr * n + 3 * k, *sh = ssh + rr * mp + k;
      if (rr < nr) {
        const double x0 = d[0], x1 = d[1], x2 = d[2], f = sz[e] * cs[k];
        const double inv = fast_rsqrt(x0 * x0 + x1 * x1 + x2 * x2);
        d[0] = x0 * inv; d[1] = x1 * inv; d[2] = x2 * inv;
        const double *u = sU + 12 * k;
#pragma unroll
        for (int i = 0; i < 4; ++i) sh[i * PL] = f * (x0 * u[i] + x1 * u[4 + i] + x2 * u[8 + i]);
      } else {  // rows past the end contribute zeros
        d[0] = d[1] = d[2] = 0.0;
        sh[0] = sh[PL] = sh[2 * PL] = sh[3 * PL] = 0.0;
      }
    }
    wave_sync();
    for (int e = lane; e < ROWS_PER_STEP * 4; e += 64) {  // V4[row][i] = (sum of the images' shares) / sigma_i
      const int i = e / ROWS_PER_STEP, rr = e - i * ROWS_PER_STEP;
      const double *sh = ssh + i * PL + rr * mp;
      double t = 0.0;
      for (int k = 0; k < m; ++k) t += sh[k];
      sv[4 * rr + i] = t * isg[i];
    }
    wave_sync();
#pragma unroll
    for (int g = 0; g < ROWS_PER_STEP / 4; ++g) {
      const int row = 4 * g + lk;
      const double v4r = sv[4 * row + i3] * use, live = row < nr ? one12 : 0.0;
      const double *xh = sx + row * n + c3;
#pragma unroll
      for (int k = 0; k < M; ++k) {
        const double val = fma(v4r, xh[3 * k], live);
        acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(val, val, acc[k], 0, 0, 0);
      }
    }
    wave_sync();  // (the operands have been read before the next step's rows overwrite them)
  }
  double *o = part + ((size_t)(blockIdx.x * 4 + wave) * m) * 256;
#pragma unroll
  for (int k = 0; k < M; ++k) {
#pragma unroll
    for (int r = 0; r < 4; ++r) o[(size_t)k * 256 + r * 64 + lane] = acc[k][r];
  }
}

// ... -> G12[k][12][12] (symmetric, index (i, c) = 3 i + c) and colsum[k][12]: one wave per entry, the partials in order
__global__ void k_dual_reduce_mfma(const double *__restrict__ part, int slots, int m, double *__restrict__ G12, double *__restrict__ colsum) {
  const int t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= m * 90) return;
  const int k = t / 90, e = t - 90 * k;  // e < 78: entry (i <= j) of the 12 x 12 matrix; else column sum e - 78
  int i = 0, j = 0;
  if (e < 78) {
    int rem = e;
    while (rem >= 12 - i) { rem -= 12 - i; ++i; }
    j = i + rem;
  } else {
    i = 12; j = e - 78;  // row 12 of the tile = sum over the rows of 1 x Z[.][j]
  }
  const double v = wave_strided_sum(part + (size_t)k * 256 + tile_elem(i, j), slots, (size_t)m * 256, lane);
  if (lane) return;
  if (e < 78) {
    G12[(size_t)k * 144 + i * 12 + j] = v;
    G12[(size_t)k * 144 + j * 12 + i] = v;
  } else {
    colsum[(size_t)k * 12 + j] = v;
  }
}

// dual scheme, pass 4 (k_dual_apply) with S formed on the fly; z in place; per block the per-image sums of (x z')^2 of the NEW depths
// (the image count stays a run-time value HERE: with it at compile time hipcc hoists the LDS reads of all M unrolled iterations --
// the w and U rows, 24 doubles per image -- in front of the loop: 256 registers + 400-600 bytes of scratch, 2.0 ms instead of 0.5)
__global__ __launch_bounds__(256, 2) void k_dual_apply_xz(const double *__restrict__ X, const double *__restrict__ cs, double is0, double is1, double is2,
                                                       double is3, const double *__restrict__ Mr, const double *__restrict__ w12,
                                                       long long n_rows, int m, double *__restrict__ z, double *__restrict__ Epart,
                                                       double *__restrict__ gpart /*[blocks][m]*/) {
  extern __shared__ double sm[];  // U4 [3m][4], w [m][12], then one tile of 64 x [3m values | m depths] per wave
  double *sU = sm, *sW = sm + 12 * (size_t)m;
  for (int q = threadIdx.x; q < 12 * m; q += blockDim.x) { sU[q] = Mr[q]; sW[q] = w12[q]; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = 3 * m, ldt = (n + m) | 1;
  double *tile = sm + 24 * (size_t)m + (size_t)wave * 64 * ldt;
  double esum = 0.0, gs[FZ_MAXM];
#pragma unroll
  for (int k = 0; k < FZ_MAXM; ++k) gs[k] = 0.0;
  for (long long base = ((long long)blockIdx.x * 4 + wave) * 64; base < n_rows; base += (long long)gridDim.x * 256) {
    const int rows_here = (int)min<long long>(64, n_rows - base);
    tile_load(X, base, rows_here, n, tile, ldt, lane);
    tile_load(z, base, rows_here, m, tile + n, ldt, lane);
    wave_sync();
    if (lane < rows_here) {
      const double *xr = tile + lane * ldt;
      double *zr = tile + lane * ldt + n;
      double s[4] = {0, 0, 0, 0};
      for (int k = 0; k < m; ++k) {
        const double x0 = xr[3 * k], x1 = xr[3 * k + 1], x2 = xr[3 * k + 2], f = zr[k] * cs[k];
        const double *u = sU + 12 * k;
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = fma(f, x0 * u[i] + x1 * u[4 + i] + x2 * u[8 + i], s[i]);
      }
      const double v4[4] = {s[0] * is0, s[1] * is1, s[2] * is2, s[3] * is3};
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < FZ_MAXM; ++k) {  // (fully unrolled: gs[] stays in registers)
        if (k < m) {
        const double x0 = xr[3 * k], x1 = xr[3 * k + 1], x2 = xr[3 * k + 2];
        const double n2 = x0 * x0 + x1 * x1 + x2 * x2, inv = fast_rsqrt(n2);
        const double xi = dual_xi(v4, x0, x1, x2, inv, sW + 12 * k);
        sum += xi;
        const double zn = xi * inv;
        zr[k] = zn;
        gs[k] = fma(zn * zn, n2, gs[k]);  // (the row's sign flip below does not change it)
        esum += reproj_err2(sU + 12 * k, s, x0, x1, x2);
        }
      }
      if (sum < 0.0)
        for (int k = 0; k < m; ++k) zr[k] = -zr[k];  // ref :217
    }
    wave_sync();
    tile_store(z, base, rows_here, m, tile + n, ldt, lane);
    wave_sync();
  }
  block_sum_to(esum, Epart);
  // the m per-image sums: a fixed shuffle tree per wave, the four waves added in order by one thread per image -- two barriers
  // (m block-wide trees of eight barriers each were a tenth of this kernel: a block lives for ten rows per thread)
  __shared__ double s_gs[4][FZ_MAXM];
#pragma unroll
  for (int k = 0; k < FZ_MAXM; ++k) {
    if (k < m) {  // (m is uniform)
      double v = gs[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) s_gs[wave][k] = v;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < m) gpart[threadIdx.x * (size_t)gridDim.x + blockIdx.x] = (s_gs[0][threadIdx.x] + s_gs[1][threadIdx.x]) + (s_gs[2][threadIdx.x] + s_gs[3][threadIdx.x]);
}
