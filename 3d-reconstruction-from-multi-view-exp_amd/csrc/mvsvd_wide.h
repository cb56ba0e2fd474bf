// Wide matrices (n > WIDE_MIN columns): block power iteration with Rayleigh-Ritz on W^T W applied implicitly -- kernels, gfx950.
// Included by mvsvd.hip inside its device-code namespace, after mvsvd_gram.h (svd_d4; the iteration's small Gram products and
// rotations are that header's kernels).  Reached from mvsvd_run / mvsvd_factorize / mvsvd_run_scaled and mvsvd_depth_step
// whenever the workspace is wide (run_wide in mvsvd.hip).
// The n x n eigenproblem of the Gram route runs in ONE workgroup: 0.4 s at n = 256, 3.3 s at 512, minutes beyond -- and its
// projection staged 5 n doubles in LDS, so that n >= ~900 did not launch at all (round 5, tools/time_svd_wide.py).  The
// callers only ever keep r <= 4 triplets (ref lib/factorization.py:10-15), so beyond WIDE_MIN columns (and up to 16 triplets) the leading subspace is
// found by block power iteration with Rayleigh-Ritz on W^T W applied IMPLICITLY, WB = 32 vectors wide, two passes over W per
// iteration and no n x n matrix anywhere:
//   B = (W - mu) Q           k_wq    (N x WB, f64 matrix cores, W staged through LDS in 64 x 64 tiles)
//   H = B^T B = Q^T W^T W Q  the fused small Gram kernel on B; Jacobi (k_jacobi_small) -> theta, Y
//   Z = (W - mu)^T (B Y)     k_rotate_rows on B, then k_wtb (n x WB, partial sums per row chunk, fixed-order reduction)
//   Q <- Q Y                 k_ritz  (Ritz vectors; residuals ||z_j - theta_j q_j||)
//   Q <- orth(Z)             Gram of Z (n x WB), Cholesky-QR in Ritz order (k_chol_orth + k_rotate_rows), twice
// Convergence factor per iteration (sigma_33 / sigma_r)^2; a measurement matrix (rank 3-4 + noise) converges in 3-6 iterations.
// The products are formed from W itself, never from an accumulated Gram matrix, and the basis is kept GRADED (Ritz order,
// triangular orthogonalisation), so a small sigma_r keeps the accuracy of the two-pass form (rounding ~ eps sigma_1 sigma_r, not
// eps sigma_1^2).  At the end B = (W - mu) Q once more: its Gram matrix is nearly diagonal and graded, a last Jacobi gives
// sigma = sqrt(theta) and the final rotation, S is B's leading columns (S = M^T W by construction: no projection pass).
// sigma[WB..] is not computed (NaN).
constexpr int MVSVD_MAX_COLS = 3 * 4096;  // three rows of W per image at MAX_CAMERAS of the bundle-adjustment engine
constexpr int WT = 64;       // tile edge of the two products

// The two products share their staging: a 64 x 64 tile of W (kept in its own dtype; converted and centred as the MFMA operand is
// read) and a 64 x WB tile of the other factor, fetched with 16-byte loads into REGISTERS while the previous tile is multiplied
// and put into LDS behind a barrier (the first version loaded element by element, stored doubles and waited for every tile's
// loads before its products: 0.9 / 1.6 TB/s on fp32 / fp64 input).  VEC: the rows of W are 16-byte aligned (n a multiple of
// 16 / sizeof(T)); otherwise the same tile comes in element by element.
template <typename T>
struct WideTile {
  static constexpr int VEC = 16 / (int)sizeof(T);          // elements per 16-byte load
  static constexpr int LD = WT + VEC;                       // padded row of the W tile (keeps 16-byte alignment)
  static constexpr int NV = WT * WT / VEC / 256;            // 16-byte loads per thread and W tile (4 / 8)
  typedef T vec_t __attribute__((ext_vector_type(16 / sizeof(T))));
  vec_t w[NV];
  double2 o[WT * WB / 2 / 256];                             // the other factor's tile: 4 loads of two doubles per thread
  // W tile rows r0 .. r0 + 63 (below r_end), columns c0 .. c0 + 63 (below n)
  __device__ __forceinline__ void load_w(const T *__restrict__ Wt, long long r0, long long r_end, int c0, int n, bool vec) {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int v = threadIdx.x + 256 * u, r = v / (WT / VEC), c = (v % (WT / VEC)) * VEC;
      const long long row = r0 + r;
      if (vec && row < r_end && c0 + c < n) {
        w[u] = *reinterpret_cast<const vec_t *>(Wt + row * n + c0 + c);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) w[u][e] = (row < r_end && c0 + c + e < n) ? Wt[row * n + c0 + c + e] : (T)0;
      }
    }
  }
  // 64 rows x WB doubles from a row-major [.][WB] matrix, rows k0 .. k0 + 63 (below k_end)
  __device__ __forceinline__ void load_o(const double *__restrict__ O, long long k0, long long k_end) {
#pragma unroll
    for (int u = 0; u < WT * WB / 2 / 256; ++u) {
      const int v = threadIdx.x + 256 * u, r = v / (WB / 2), c = (v % (WB / 2)) * 2;
      o[u] = (k0 + r < k_end) ? *reinterpret_cast<const double2 *>(O + (k0 + r) * WB + c) : double2{0.0, 0.0};
    }
  }
  __device__ __forceinline__ void store(T (*sW)[LD], double (*sO)[WB + 2]) const {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int v = threadIdx.x + 256 * u, r = v / (WT / VEC), c = (v % (WT / VEC)) * VEC;
      *reinterpret_cast<vec_t *>(&sW[r][c]) = w[u];
    }
#pragma unroll
    for (int u = 0; u < WT * WB / 2 / 256; ++u) {
      const int v = threadIdx.x + 256 * u, r = v / (WB / 2), c = (v % (WB / 2)) * 2;
      *reinterpret_cast<double2 *>(&sO[r][c]) = o[u];
    }
  }
};

// B[row][j] = sum_c (Wt[row][c] - mu[c]) Q[c][j], j < WB.  One workgroup per 64 rows, wave w its rows 16 w .. 16 w + 15.
template <typename T>
__global__ __launch_bounds__(256) void k_wq(const T *__restrict__ Wt, long long n_rows, int n, const double *__restrict__ mu,
                                            const double *__restrict__ Q, double *__restrict__ B) {
  typedef WideTile<T> Tile;
  __shared__ __attribute__((aligned(16))) T sW[WT][Tile::LD];
  __shared__ __attribute__((aligned(16))) double sQ[WT][WB + 2];
  __shared__ double smu[WT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const long long r0 = (long long)blockIdx.x * WT;
  const bool vec = n % Tile::VEC == 0;
  svd_d4 acc[2] = {svd_d4{0, 0, 0, 0}, svd_d4{0, 0, 0, 0}};
  Tile t;
  t.load_w(Wt, r0, n_rows, 0, n, vec);
  t.load_o(Q, 0, n);
  for (int c0 = 0; c0 < n; c0 += WT) {
    __syncthreads();  // the previous tile's products are done
    t.store(sW, sQ);
    if (threadIdx.x < WT) smu[threadIdx.x] = (mu && c0 + (int)threadIdx.x < n) ? mu[c0 + threadIdx.x] : 0.0;
    __syncthreads();
    if (c0 + WT < n) {  // the next tile's loads fly under this tile's products
      t.load_w(Wt, r0, n_rows, c0 + WT, n, vec);
      t.load_o(Q, c0 + WT, n);
    }
#pragma unroll
    for (int kk = 0; kk < WT / 4; ++kk) {
      const int k = 4 * kk + lk;
      const double a = (double)sW[16 * wave + li][k] - smu[k];
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sQ[k][li], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sQ[k][16 + li], acc[1], 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long row = r0 + 16 * wave + lk + 4 * q;
    if (row < n_rows) {
      B[row * WB + li] = acc[0][q];
      B[row * WB + 16 + li] = acc[1][q];
    }
  }
}

// zpart[chunk][c][j] = sum over the chunk's rows of (Wt[row][c] - mu[c]) B[row][j].  blockIdx.x = 64 columns of W (wave w its
// columns 16 w ..), blockIdx.y = row chunk (rows_per_chunk, a multiple of 64).
template <typename T>
__global__ __launch_bounds__(256) void k_wtb(const T *__restrict__ Wt, long long n_rows, int n, const double *__restrict__ mu,
                                             const double *__restrict__ B, long long rows_per_chunk, double *__restrict__ zpart) {
  typedef WideTile<T> Tile;
  __shared__ __attribute__((aligned(16))) T sW[WT][Tile::LD];
  __shared__ __attribute__((aligned(16))) double sB[WT][WB + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const int c0 = blockIdx.x * WT;
  const long long rb = (long long)blockIdx.y * rows_per_chunk, re = min(n_rows, rb + rows_per_chunk);
  const bool vec = n % Tile::VEC == 0;
  const int ca = min(c0 + 16 * wave + li, n - 1);
  const double mua = mu ? mu[ca] : 0.0;  // this lane's column of W
  svd_d4 acc[2] = {svd_d4{0, 0, 0, 0}, svd_d4{0, 0, 0, 0}};
  Tile t;
  if (rb < re) {
    t.load_w(Wt, rb, re, c0, n, vec);
    t.load_o(B, rb, re);
  }
  for (long long r0 = rb; r0 < re; r0 += WT) {
    __syncthreads();
    t.store(sW, sB);
    __syncthreads();
    if (r0 + WT < re) {
      t.load_w(Wt, r0 + WT, re, c0, n, vec);
      t.load_o(B, r0 + WT, re);
    }
    const int rows_here = (int)min<long long>(WT, re - r0);  // (a zero row of W is -mu after centring: the rows past the end must not count)
#pragma unroll
    for (int kk = 0; kk < WT / 4; ++kk) {
      const int k = 4 * kk + lk;
      const double a = k < rows_here ? (double)sW[k][16 * wave + li] - mua : 0.0;  // A[i][k] = W[row k][column i]
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sB[k][li], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sB[k][16 + li], acc[1], 0, 0, 0);
    }
  }
  double *out = zpart + (size_t)blockIdx.y * n * WB;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = c0 + 16 * wave + lk + 4 * q;
    if (c < n) {
      out[(size_t)c * WB + li] = acc[0][q];
      out[(size_t)c * WB + 16 + li] = acc[1][q];
    }
  }
}

// out[e] = sum over the chunks, in order, of part[chunk][e]
__global__ void k_sum_chunks(const double *__restrict__ part, int chunks, long long count, double *__restrict__ out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  double s = 0.0;
  int c = 0;
  for (; c + 8 <= chunks; c += 8) {  // eight loads in flight, added in order (one load per trip waited a memory latency per chunk: 0.14 ms at 400 chunks)
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(c + u) * count + e];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; c < chunks; ++c) s += part[(size_t)c * count + e];
  out[e] = s;
}

// Q[n][WB]: a fixed pseudo-random start (the same for every call: the result must not depend on a seed the caller cannot see)
__device__ __forceinline__ double wide_hash(unsigned long long x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return (double)(long long)(x >> 11) * (1.0 / 4503599627370496.0) - 1.0;  // [-1, 1)
}
__global__ void k_wide_init(double *__restrict__ Q, int n, unsigned long long salt) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (long long)n * WB) Q[e] = wide_hash((unsigned long long)e * 0x9e3779b97f4a7c15ull + salt);
}

// Ritz rotation of the basis, one thread per row: q <- q Y (Y = eigenvectors of H; `Hr` = Y^T H Y as the small solver leaves it:
// theta on the diagonal, whatever it did not rotate away beside it), and the residual partials
// respart[block][j] = sum_rows (z_j - sum_i q_i Hr_ij)^2 against Z = W^T (B Y), which the caller formed from the ROTATED product.
//  * Rotating Z itself -- z <- z Y -- forms a vector of length sigma_4^2 as a combination of vectors of length sigma_1^2: a
//    sigma_4 = 1e-7 sigma_1 then comes out with 1e-16 / 1e-14 of relative noise, most of it outside the row space of W, and the
//    block loses that direction to 2e-3 (found with a NumPy restatement of the iteration).  B Y loses 1e-16 / 1e-7 and W^T maps
//    whatever it is given into the row space.
//  * The residual is taken against the WHOLE row of Hr, not theta_j alone: the solver leaves |Hr_1j| up to 4.5e-16 theta_1 (its
//    absolute floor), i.e. q_j keeps 1e-16 of q_1 -- harmless for q_j, but theta_1 times it is 1e-2 of a theta_j = 1e-14 theta_1
//    and would sit in the plain residual for ever.  Projected (the Galerkin condition, numerically), what is left is the part of
//    W^T W q_j OUTSIDE the block: the quantity the next iteration can still improve.
// Z == nullptr: the rotation alone.
__global__ __launch_bounds__(256) void k_ritz(double *__restrict__ Q, const double *__restrict__ Z, int n, const double *__restrict__ Y,
                                              const double *__restrict__ Hr, double *__restrict__ respart) {
  __shared__ double sY[WB][WB], sH[WB][WB], sred[4][WB];
  for (int e = threadIdx.x; e < WB * WB; e += 256) { sY[e >> 5][e & 31] = Y[e]; sH[e >> 5][e & 31] = Hr[e]; }
  __syncthreads();
  const int row = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool ok = row < n;
  double q[WB];
#pragma unroll
  for (int k = 0; k < WB; ++k) q[k] = ok ? Q[(size_t)row * WB + k] : 0.0;
#pragma unroll 1
  for (int j = 0; j < WB; ++j) {
    double qj = 0.0;
#pragma unroll
    for (int k = 0; k < WB; ++k) qj = fma(q[k], sY[k][j], qj);
    if (ok) Q[(size_t)row * WB + j] = qj;
  }
  if (!Z || !respart) return;  // (uniform)
#pragma unroll
  for (int k = 0; k < WB; ++k) q[k] = ok ? Q[(size_t)row * WB + k] : 0.0;  // the rotated row (this thread's own stores)
#pragma unroll 1
  for (int j = 0; j < WB; ++j) {
    double zp = 0.0;
#pragma unroll
    for (int k = 0; k < WB; ++k) zp = fma(q[k], sH[k][j], zp);
    double d = (ok ? Z[(size_t)row * WB + j] : 0.0) - zp;
    d *= d;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) d += __shfl_down(d, off, 64);
    if (lane == 0) sred[wave][j] = d;
  }
  __syncthreads();
  if (threadIdx.x < WB) respart[(size_t)blockIdx.x * WB + threadIdx.x] = (sred[0][threadIdx.x] + sred[1][threadIdx.x]) + (sred[2][threadIdx.x] + sred[3][threadIdx.x]);
}

// Orthonormalisation step: Cholesky-QR in Ritz order.  The columns of Z differ in length by (sigma_1 / sigma_32)^2, so C = Z^T Z
// is brought to unit diagonal (d_j = C_jj^-1/2: its entries are then accurate to eps whatever the columns' lengths), its rows and
// columns are put in the order of DESCENDING Ritz value (`Hd`: the diagonal the small solver left in H; nullptr: as they are), and
// P^T D C D P = L L^T.  Q = Z D P L^-T then has orthonormal columns, sorted by Ritz value, and column r only mixes the columns of
// rank <= r -- a small triplet's vector is cleaned of the large ones and never the other way round, so the basis stays graded
// and the next Rayleigh-Ritz step keeps the small triplets' relative accuracy.  (A symmetric orthogonalisation -- eigenvectors of C --
// mixes every column with the 28 noise columns at the 1 / sqrt(n) level: B^T B was then no longer graded, a sigma_4 = 1e-7 sigma_1
// came out of the Ritz step to 1e-2 only, and the residual test stalled there.)  A pivot below 1e-12 -- the column depends on
// its predecessors to 1e-6: the block has lost rank, W has fewer than WB independent rows / columns, or a column of Z is exactly
// zero -- gives a zero column and flag[r] = 1; k_wide_refill then puts a pseudo-random column in its place before the second pass.
// One wave; lane i owns row i of the factor.
__global__ __launch_bounds__(64) void k_chol_orth(const double *__restrict__ C, const double *__restrict__ Hd, double *__restrict__ Tm,
                                                  int *__restrict__ flag) {
  __shared__ double A[WB][WB + 1], Li[WB][WB + 1], sd[WB], sth[WB];
  __shared__ int perm[WB], dead[WB];
  const int lane = threadIdx.x;
  if (lane < WB) {
    const double c = C[lane * WB + lane];
    sd[lane] = c > 0.0 ? 1.0 / sqrt(c) : 0.0;
    sth[lane] = Hd ? Hd[lane * WB + lane] : 0.0;
  }
  __syncthreads();
  if (lane < WB) {  // rank of this column by Ritz value (ties: by index)
    int r = 0;
    for (int k = 0; k < WB; ++k) r += (sth[k] > sth[lane]) || (sth[k] == sth[lane] && k < lane);
    perm[Hd ? r : lane] = lane;
  }
  __syncthreads();
  for (int e = lane; e < WB * WB; e += 64) {
    const int i = e >> 5, j = e & 31, pi = perm[i], pj = perm[j];
    A[i][j] = i == j ? (sd[pi] > 0.0 ? 1.0 : 0.0) : C[pi * WB + pj] * sd[pi] * sd[pj];
    Li[i][j] = 0.0;
  }
  __syncthreads();
  // right-looking Cholesky, the factor overwrites the lower triangle of A
  for (int j = 0; j < WB; ++j) {
    if (lane == j) {
      const double piv = A[j][j];
      dead[j] = !(piv > 1e-12);
      A[j][j] = dead[j] ? 1.0 : sqrt(piv);
    }
    __syncthreads();
    const bool dj = dead[j] != 0;
    if (lane > j && lane < WB) A[lane][j] = dj ? 0.0 : A[lane][j] / A[j][j];
    __syncthreads();
    if (lane > j && lane < WB && !dj) {
      const double lij = A[lane][j];
      for (int k = j + 1; k <= lane; ++k) A[lane][k] -= lij * A[k][j];
    }
    __syncthreads();
  }
  // L^-1 by forward substitution, lane c its column c
  if (lane < WB) {
    const int c = lane;
    for (int i = c; i < WB; ++i) {
      double v = i == c ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) v -= A[i][k] * Li[k][c];
      Li[i][c] = v / A[i][i];
    }
  }
  __syncthreads();
  // T[p_i][r] = d_{p_i} (L^-1)[r][i], i <= r
  for (int e = lane; e < WB * WB; e += 64) {
    const int i = e >> 5, r = e & 31;
    Tm[perm[i] * WB + r] = (i <= r && !dead[r]) ? sd[perm[i]] * Li[r][i] : 0.0;
  }
  if (lane < WB) flag[lane] = dead[lane];
}
__global__ void k_wide_refill(double *__restrict__ Q, int n, const int *__restrict__ flag, unsigned long long salt) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)n * WB) return;
  const int j = (int)(e & (WB - 1));
  if (flag[j]) Q[e] = wide_hash((unsigned long long)e * 0x9e3779b97f4a7c15ull + salt) * rsqrt((double)n / 3.0);  // ~unit length
}

// S[i][row] = sgn[i] B[row][col[i]] (the workspace's dtype): the leading columns of the rotated B ARE M^T (W - mu)
template <typename T>
__global__ void k_take_cols(const double *__restrict__ B, long long n_rows, int r, const int *__restrict__ col, const double *__restrict__ sgn, T *__restrict__ S) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  for (int i = 0; i < r; ++i) S[(size_t)i * n_rows + row] = (T)(sgn[i] * B[row * WB + col[i]]);
}
