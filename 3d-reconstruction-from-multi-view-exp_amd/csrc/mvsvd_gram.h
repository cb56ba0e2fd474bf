// The Gram route of the thin SVD (K7a, K7d) -- kernels, gfx950: G = (Wt - mu)^T (Wt - mu) on the f64 matrix cores with its
// two-level fixed-order reduction, the column means, and the rotations B = (Wt - mu) V.
// Included by mvsvd.hip inside its device-code namespace, first of the mvsvd_*.h headers: uses svd_d4 and GRAM_SLICES of
// mvsvd.hip and the tile sizes of mvba_host.h (GT, ROWS_PER_STEP, GRAM_ROWS); gram_store_partial and tile_elem also serve the
// fused depth route (mvsvd_depth_fused.h).  Reached from mvsvd_run / mvsvd_factorize / mvsvd_run_scaled and the wide path's small
// Gram products through launch_gram_n, gram_reduce_finish, column_means, launch_rotate and launch_rotate_rows in mvsvd.hip.

// G += Wt^T Wt on the f64 matrix cores.  For 4 consecutive rows r0..r3 and column tiles (ti,tj):
//   A[i][k] = Wt[r_k][16 ti + i]   (lane l: i = l & 15, k = l >> 4)
//   B[k][j] = Wt[r_k][16 tj + j]   (lane l: k = l >> 4, j = l & 15)
// so both operands are "this lane's row (l >> 4), this lane's column (l & 15) of a tile": one
// value per lane per tile, converted to fp64 on load.  C/D: col = l & 15, row = (l >> 4) + 4 reg.
// Partial tiles go to partial[chunk][pair][256] (no atomics: millions of f64 adds onto a
// 24 x 24 matrix serialise at the memory side); k_gram_reduce sums the chunks in fixed order.
// `red`: npairs x 8 KiB of LDS the caller no longer needs (24 KiB of STATIC shared memory here once held a block of the
// fused kernel to 36 KiB: four blocks per CU instead of eight, one wave per SIMD too few to keep the matrix core fed)
__device__ __forceinline__ void gram_store_partial(const svd_d4 *acc, int npairs, int pair0, int pairs_total,
                                                   double *__restrict__ partial, double *red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = 0; q < npairs; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[((wave * npairs + q) * 4 + r) * 64 + lane] = acc[q][r];
  __syncthreads();
  double *out = partial + ((size_t)blockIdx.y * pairs_total + pair0) * 256;
  for (int e = threadIdx.x; e < npairs * 256; e += 256) {
    const int q = e >> 8, rl = e & 255;  // rl = r * 64 + lane
    out[e] = (red[((0 * npairs + q) << 8) + rl] + red[((1 * npairs + q) << 8) + rl]) + (red[((2 * npairs + q) << 8) + rl] + red[((3 * npairs + q) << 8) + rl]);
  }
}

// n <= 32: one pass over the rows forms every tile pair.  MODE 1: n <= 16, one MFMA per 4 rows.  MODE 3: 24 < n <= 32,
// the three tile pairs (0,0), (0,1), (1,1).  MODE 2: 16 < n <= 24 (config 5: 24 columns), TWO MFMAs: tile (0,0) and a
// PACKED tile whose rows are columns 8..23 and whose columns are [16..23 | 0..7] -- it holds G[8..23][16..23] and
// G[16..23][0..7], i.e. everything tile (0,0) lacks; the half-empty (0,1) and quarter-full (1,1) tiles of MODE 3 cost a
// third more matrix-core time for the same 300 entries (the kernel is bound by the f64 MFMA issue rate).
// A workgroup takes GRAM_ROWS consecutive rows per step: the rows are one contiguous byte range of
// Wt, streamed with 16-byte loads by all 256 threads into LDS (a lane-per-element gather of the
// MFMA operands straight from HBM ran at 1.8 TB/s), then every wave picks the operands of its
// 32 rows out of LDS.  Rows past the end are zero-filled in LDS.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_gram_fused(const T *__restrict__ Wt, long long n_rows, int n,
                                                    const double *__restrict__ mu, double *__restrict__ partial) {
  extern __shared__ double gram_lds_raw[];
  T *stage = reinterpret_cast<T *>(gram_lds_raw);  // GRAM_ROWS x n, row-major like Wt
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  constexpr int NP = MODE == 1 ? 1 : (MODE == 2 ? 2 : 3);  // MFMAs per 4 rows = partial tiles
  constexpr int NC = MODE == 1 ? 1 : (MODE == 2 ? 3 : 2);  // operand columns a lane reads per row
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(VEC)));
  svd_d4 acc[3] = {svd_d4{0, 0, 0, 0}, svd_d4{0, 0, 0, 0}, svd_d4{0, 0, 0, 0}};
  int col[NC];
  bool cok[NC];
  double muc[NC];  // column mean to subtract (0 without centring)
#pragma unroll
  for (int t = 0; t < NC; ++t) {
    // MODE 1/3: column 16 t + li.  MODE 2: li | 8 + li | (li < 8 ? 16 + li : li - 8)
    const int c = MODE == 2 ? (t == 0 ? li : (t == 1 ? 8 + li : (li < 8 ? 16 + li : li - 8))) : GT * t + li;
    cok[t] = c < n; col[t] = min(c, n - 1); muc[t] = mu ? mu[col[t]] : 0.0;
  }
  // (PMC: the general operand path -- subtract the mean, mask absent columns and rows past the end -- was 12 vector
  // instructions per MFMA, 122 M issue cycles next to 160 M of matrix-core time, and the two did not overlap)
  const bool lean = mu == nullptr && n == (MODE == 1 ? 16 : (MODE == 2 ? 24 : 32));
  const long long total = n_rows * n;
  const int nvec = GRAM_ROWS * n / VEC;  // GRAM_ROWS * n is a multiple of 4
  constexpr int MAXV = GRAM_ROWS * 32 / VEC / 256;  // n <= 32: at most this many vectors per thread
  vec_t xs[MAXV];
  auto load_step = [&](long long r0) {  // every load of a step is issued before anything waits for one
    const long long e0 = r0 * n;        // first element of the step: 16-byte aligned (r0 is a multiple of 128)
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
      const int v = threadIdx.x + 256 * u;
      const long long idx = e0 + (long long)v * VEC;
      if (v < nvec && idx + VEC <= total) {
        xs[u] = *reinterpret_cast<const vec_t *>(Wt + idx);
      } else {
#pragma unroll
        for (int w = 0; w < VEC; ++w) xs[u][w] = (v < nvec && idx + w < total) ? Wt[idx + w] : (T)0;
      }
    }
  };
  const long long r_first = (long long)blockIdx.y * GRAM_ROWS, r_stride = (long long)gridDim.y * GRAM_ROWS;
  if (r_first < n_rows) load_step(r_first);
  for (long long r0 = r_first; r0 < n_rows; r0 += r_stride) {
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
      const int v = threadIdx.x + 256 * u;
      if (v < nvec) *reinterpret_cast<vec_t *>(stage + (size_t)v * VEC) = xs[u];
    }
    __syncthreads();
    if (r0 + r_stride < n_rows) load_step(r0 + r_stride);  // the next step's rows travel while this step's are multiplied
    const T *rows = stage + (size_t)(wave * ROWS_PER_STEP + lk) * n;
    const long long row0 = r0 + wave * ROWS_PER_STEP + lk;
#pragma unroll
    for (int g = 0; g < ROWS_PER_STEP / 4; ++g) {
      double v[NC];
      if (lean) {  // (uniform) no centring, every operand column exists: a row past the end is zeros in LDS and stays zero
#pragma unroll
        for (int t = 0; t < NC; ++t) v[t] = (double)rows[(4 * g) * n + col[t]];
      } else {
        const bool rok = row0 + 4 * g < n_rows;  // rows past the end are zeros in LDS: keep them zero when centring
#pragma unroll
        for (int t = 0; t < NC; ++t) {
          const double x = (double)rows[(size_t)(4 * g) * n + col[t]] - muc[t];
          v[t] = (cok[t] && rok) ? x : 0.0;
        }
      }
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
    __syncthreads();
  }
  gram_store_partial(acc, NP, 0, NP, partial, gram_lds_raw);  // (the staging buffer: the last step ended with a barrier)
}

// larger n: blockIdx.x = one upper tile pair (the rows are re-read once per pair, from L2 / MALL)
template <typename T>
__global__ __launch_bounds__(256) void k_gram_pair(const T *__restrict__ Wt, long long n_rows, int n, int n_tiles,
                                                   int n_pairs, const double *__restrict__ mu, double *__restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  int ti = 0, pr = blockIdx.x;
  while (pr >= n_tiles - ti) { pr -= n_tiles - ti; ++ti; }
  const int tj = ti + pr;
  const bool aok = GT * ti + li < n, bok = GT * tj + li < n;
  const int ca = min(GT * ti + li, n - 1), cb = min(GT * tj + li, n - 1);
  const double mua = mu ? mu[ca] : 0.0, mub = mu ? mu[cb] : 0.0;
  svd_d4 acc[3] = {svd_d4{0, 0, 0, 0}, svd_d4{0, 0, 0, 0}, svd_d4{0, 0, 0, 0}};
  const long long stride = (long long)gridDim.y * 4 * ROWS_PER_STEP;
  for (long long r0 = ((long long)blockIdx.y * 4 + wave) * ROWS_PER_STEP; r0 < n_rows; r0 += stride) {
    double va[ROWS_PER_STEP / 4], vb[ROWS_PER_STEP / 4];
#pragma unroll
    for (int g = 0; g < ROWS_PER_STEP / 4; ++g) {
      const long long row = r0 + 4 * g + lk;
      const T *wr = Wt + min(row, n_rows - 1) * n;
      const double xa = (double)wr[ca] - mua, xb = (double)wr[cb] - mub;
      va[g] = (row < n_rows && aok) ? xa : 0.0;
      vb[g] = (row < n_rows && bok) ? xb : 0.0;
    }
#pragma unroll
    for (int g = 0; g < ROWS_PER_STEP / 4; ++g) acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[g], vb[g], acc[0], 0, 0, 0);
  }
  __shared__ double red1[4 * 4 * 64];
  gram_store_partial(acc, 1, blockIdx.x, n_pairs, partial, red1);
}

// Two fixed-order levels instead of atomics: k_gram_reduce sums a slice of the row chunks per block
// (slice s of tile pair p -> part2[s][p][256]), k_gram_finish adds the slices in order and writes the full symmetric G.
__global__ __launch_bounds__(256) void k_gram_reduce(const double *__restrict__ partial, int chunks, int n_pairs,
                                                     double *__restrict__ part2) {
  const int e = threadIdx.x;
  double sacc = 0.0;  // gridDim.y slices of the chunk range, 8 independent loads in flight
  const int c0 = (int)((long long)chunks * blockIdx.y / gridDim.y), c1 = (int)((long long)chunks * (blockIdx.y + 1) / gridDim.y);
#pragma unroll 8
  for (int c = c0; c < c1; ++c) sacc += partial[((size_t)c * n_pairs + blockIdx.x) * 256 + e];
  part2[((size_t)blockIdx.y * n_pairs + blockIdx.x) * 256 + e] = sacc;
}

// element (row, col) of a 16 x 16 MFMA C/D tile as gram_store_partial lays it out: col = l & 15, row = (l >> 4) + 4 reg
__device__ __forceinline__ int tile_elem(int row, int col) { return ((row >> 2) << 6) | ((row & 3) << 4) | col; }

// G[i][j] = G[j][i] = sum over the slices (in order) of the tile entry that holds it.  `packed`: the two-tile layout
// of k_gram_fused MODE 2.  Entries a layout holds twice (both halves of a diagonal tile) are averaged.
__global__ void k_gram_finish(const double *__restrict__ part2, int slices, int n_pairs, int n_tiles, int packed,
                              double *__restrict__ G, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= n || j < i) return;
  auto fetch = [&](int pair, int elem) {  // (every load issued before the first add: one memory latency, not `slices`)
    double t[GRAM_SLICES];
#pragma unroll
    for (int s = 0; s < GRAM_SLICES; ++s) t[s] = part2[((size_t)min(s, slices - 1) * n_pairs + pair) * 256 + elem];
    double v = 0.0;
#pragma unroll
    for (int s = 0; s < GRAM_SLICES; ++s) v += s < slices ? t[s] : 0.0;
    return v;
  };
  double v;
  if (packed) {
    if (j < 16) v = (i == j) ? fetch(0, tile_elem(i, j)) : 0.5 * (fetch(0, tile_elem(i, j)) + fetch(0, tile_elem(j, i)));
    else if (i < 8) v = fetch(1, tile_elem(j - 8, 8 + i));                      // G[j][i], j >= 16 > 8 > i
    else if (i < 16) v = fetch(1, tile_elem(i - 8, j - 16));                    // G[i][j], 8 <= i < 16 <= j
    else v = (i == j) ? fetch(1, tile_elem(i - 8, j - 16)) : 0.5 * (fetch(1, tile_elem(i - 8, j - 16)) + fetch(1, tile_elem(j - 8, i - 16)));
  } else {
    const int ti = i / GT, tj = j / GT;
    const int pair = ti * n_tiles - ti * (ti - 1) / 2 + (tj - ti);
    v = fetch(pair, tile_elem(i - GT * ti, j - GT * tj));
    if (ti == tj && j > i) v = 0.5 * (v + fetch(pair, tile_elem(j - GT * tj, i - GT * ti)));  // diagonal tiles hold both halves
  }
  G[(size_t)i * n + j] = v;
  G[(size_t)j * n + i] = v;
}

// column sums (only when centring is requested): one block row per column, grid-stride over rows
template <typename T>
__global__ __launch_bounds__(256) void k_colsum(const T *__restrict__ Wt, long long n_rows, int n,
                                                double *__restrict__ colsum) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  double s = 0.0;
  for (long long r = (long long)blockIdx.y * 256 + threadIdx.x; r < n_rows; r += (long long)gridDim.y * 256)
    s += (double)Wt[r * n + c];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) colsum[(size_t)blockIdx.y * n + c] = red[0];  // one partial per (slice, column): no atomics
}

__global__ void k_mean_from_sum(const double *__restrict__ colsum, int slices, int n, long long n_rows, double *__restrict__ mu) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double s = 0.0;
  for (int q = 0; q < slices; ++q) s += colsum[(size_t)q * n + c];  // fixed order
  mu[c] = s / (double)n_rows;
}

// B[row][j] = sum_c (Wt[row][c] - mu[c]) V[c][j]   (fp64 out): the preconditioning rotation of the
// second pass, and V1 V2 at the end (rows = n).  64 x 64 output tile per block, k in steps of 16
// through LDS, 4 x 4 outputs per thread.
template <typename T>
__global__ __launch_bounds__(256) void k_rotate(const T *__restrict__ Wt, long long n_rows, int n, const double *__restrict__ mu,
                                                const double *__restrict__ V, double *__restrict__ B) {
  __shared__ double sW[64][17], sV[16][65];
  const long long r0 = (long long)blockIdx.x * 64;
  const int j0 = blockIdx.y * 64;
  const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;  // thread -> rows tr + 16 u, columns tc + 16 v
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
  for (int k0 = 0; k0 < n; k0 += 16) {
    for (int e = threadIdx.x; e < 64 * 16; e += 256) {
      const int r = e >> 4, k = e & 15;
      const long long row = r0 + r;
      sW[r][k] = (row < n_rows && k0 + k < n) ? (double)Wt[row * n + k0 + k] - (mu ? mu[k0 + k] : 0.0) : 0.0;
    }
    for (int e = threadIdx.x; e < 16 * 64; e += 256) {
      const int k = e >> 6, j = e & 63;
      sV[k][j] = (k0 + k < n && j0 + j < n) ? V[(size_t)(k0 + k) * n + j0 + j] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = sW[tr + 16 * u][k];
#pragma unroll
      for (int v = 0; v < 4; ++v) b[v] = sV[k][tc + 16 * v];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] += a[u] * b[v];
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long row = r0 + tr + 16 * u;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = j0 + tc + 16 * v;
      if (row < n_rows && j < n) B[row * n + j] = acc[u][v];
    }
  }
}

// The same product for n <= 32 columns and many rows (the preconditioning rotation of a tall matrix: 1.06 ms for 5 M x 24 with
// the generic kernel above -- 64 x 64 output tiles of which 24 columns exist, element-wise loads -- against 0.35 ms of HBM
// time for its 1.9 GB).  Built like k_gram_fused: a workgroup takes 128 consecutive rows per step, one contiguous byte range
// streamed with 16-byte loads by all threads into LDS (the next step's loads in flight during this step's products); every
// wave rotates its 32 rows on the f64 matrix cores -- A[i][k] = W[16 t + i][4 g + k] - mu, B[k][j] = V[4 g + k][16 c + j]
// (kept in registers) -- and stores the result from the MFMA output layout.
template <typename T>
__global__ __launch_bounds__(256) void k_rotate_rows(const T *__restrict__ Wt, long long n_rows, int n, const double *__restrict__ mu,
                                                     const double *__restrict__ V, double *__restrict__ B) {
  extern __shared__ double rot_lds[];
  T *stage = reinterpret_cast<T *>(rot_lds);                       // GRAM_ROWS x n, row-major like Wt
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const int nct = (n + 15) / 16, ng = (n + 3) / 4;                 // column tiles (<= 2), k-steps (<= 8)
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(VEC)));
  double vb[2][8], mk[8];                                          // this lane's B operands and the means of its k columns
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const int k = 4 * g + lk;
    mk[g] = (mu && k < n) ? mu[k] : 0.0;
#pragma unroll
    for (int c = 0; c < 2; ++c) vb[c][g] = (k < n && 16 * c + li < n) ? V[(size_t)k * n + 16 * c + li] : 0.0;
  }
  const long long total = n_rows * n;
  const int nvec = GRAM_ROWS * n / VEC;
  constexpr int MAXV = GRAM_ROWS * 32 / VEC / 256;
  vec_t xs[MAXV];
  auto load_step = [&](long long r0) {
    const long long e0 = r0 * n;
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
      const int v = threadIdx.x + 256 * u;
      const long long idx = e0 + (long long)v * VEC;
      if (v < nvec && idx + VEC <= total) {
        xs[u] = *reinterpret_cast<const vec_t *>(Wt + idx);
      } else {
#pragma unroll
        for (int w = 0; w < VEC; ++w) xs[u][w] = (v < nvec && idx + w < total) ? Wt[idx + w] : (T)0;
      }
    }
  };
  const long long r_first = (long long)blockIdx.x * GRAM_ROWS, r_stride = (long long)gridDim.x * GRAM_ROWS;
  if (r_first < n_rows) load_step(r_first);
  for (long long r0 = r_first; r0 < n_rows; r0 += r_stride) {
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
      const int v = threadIdx.x + 256 * u;
      if (v < nvec) *reinterpret_cast<vec_t *>(stage + (size_t)v * VEC) = xs[u];
    }
    __syncthreads();
    if (r0 + r_stride < n_rows) load_step(r0 + r_stride);
#pragma unroll
    for (int t = 0; t < 2; ++t) {  // the wave's two 16-row tiles
      const T *rows = stage + (size_t)(wave * ROWS_PER_STEP + 16 * t + li) * n;
      svd_d4 acc[2] = {svd_d4{0, 0, 0, 0}, svd_d4{0, 0, 0, 0}};
#pragma unroll
      for (int g = 0; g < 8; ++g) {  // (static indices into the operand registers; ng and nct are uniform)
        if (g >= ng) break;
        const int k = 4 * g + lk;
        const double a = (k < n) ? (double)rows[k] - mk[g] : 0.0;
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, vb[0][g], acc[0], 0, 0, 0);
        if (nct > 1) acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, vb[1][g], acc[1], 0, 0, 0);
      }
      // C/D layout: col = li, row = lk + 4 q: four 128-byte row segments per store instruction, straight to HBM (through a
      // second LDS buffer and contiguous 16-byte stores the kernel held two workgroups per CU and ran at 2.4 TB/s)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long long row = r0 + wave * ROWS_PER_STEP + 16 * t + lk + 4 * q;
        if (row < n_rows) {
          double *orow = B + row * n;
          if (li < n) orow[li] = acc[0][q];
          if (16 + li < n) orow[16 + li] = acc[1][q];
        }
      }
    }
    __syncthreads();  // every wave has read its rows: the staging buffer may take the next step
  }
}
