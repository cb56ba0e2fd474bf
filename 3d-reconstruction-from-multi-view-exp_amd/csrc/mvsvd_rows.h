// Kernels that walk the rows of the measurement matrix -- gfx950: the projection S = M^T W (K7c), the coalesced 64-row LDS
// tiles (tile_load / tile_store), loading images into their columns, the depth-weighted matrix W = X o z with its row or
// column-group normalisation, and the fixed-order sums (wave_strided_sum, block_sum_to) that the depth kernels share.
// Included by mvsvd.hip inside its device-code namespace, before the two depth headers.  Reached from mvsvd_run / mvsvd_factorize
// (k_project), mvsvd_load_images (k_image_cols), mvsvd_load_base_images (k_base_image), mvsvd_run_scaled and the unfused
// mvsvd_depth_step (k_group_sumsq, k_group_scale, k_scale_rows_*), mvsvd_depth_begin (k_fill).

// S[i][row] = sum_c Mr[c][i] (Wt[row][c] - mu[c]).  A wave takes 64 consecutive rows: the 64 x n
// tile is contiguous in memory, so it is loaded with fully coalesced accesses into a padded LDS
// tile (odd stride -> conflict-free column reads), then each lane reduces its own row.
template <typename T>
__global__ __launch_bounds__(256) void k_project(const T *__restrict__ Wt, long long n_rows, int n, int r,
                                                 const double *__restrict__ Mr4 /*[n][4], zero padded beyond r*/, const double *__restrict__ mu,
                                                 T *__restrict__ S) {
  extern __shared__ double sm[];  // (4 n doubles unused since the basis is read by scalar loads), mu [n], then per-wave tiles of T
  double *smu = sm + 4 * (size_t)n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nc = min(n, PC), ldt = nc | 1;  // odd stride
  T *tile = reinterpret_cast<T *>(smu + n) + (size_t)wave * 64 * ldt;
  for (int q = threadIdx.x; q < n; q += blockDim.x) smu[q] = mu ? mu[q] : 0.0;
  __syncthreads();
  const long long stride = (long long)gridDim.x * 256;
  for (long long base = (long long)blockIdx.x * 256 + 64 * wave; base < n_rows; base += stride) {
    const int rows_here = (int)min<long long>(64, n_rows - base);
    double acc[4] = {0, 0, 0, 0};
    for (int c0 = 0; c0 < n; c0 += PC) {
      const int w = min(PC, n - c0);
      if (w == n) {  // whole rows: the tile is one contiguous block of rows_here * n elements
        const T *src = Wt + base * n;
        // (batches of eight independent loads, then their LDS stores: one load and one store per trip waited for every load
        // before issuing the next: 0.43 -> 0.26 ms at 5 M x 24 fp64.  A streaming MFMA form like k_rotate_rows, its 32 x r result
        // transposed through LDS, was slower than this kernel: 0.39 ms, fp32 0.18 against 0.16)
        constexpr int U = 8;
        if (sizeof(T) == 4 && (n & 3) == 0) {  // 16 B per lane; a float4 never straddles a row
          const int n4 = n >> 2, total4 = rows_here * n4;
          const float4 *src4 = reinterpret_cast<const float4 *>(src);
          for (int q0 = lane; q0 < total4; q0 += 64 * U) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = src4[min(q0 + 64 * u, total4 - 1)];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int q = q0 + 64 * u, rr = q / n4;
              if (q < total4) {
                T *d = tile + rr * ldt + 4 * (q - rr * n4);
                d[0] = (T)v[u].x; d[1] = (T)v[u].y; d[2] = (T)v[u].z; d[3] = (T)v[u].w;
              }
            }
          }
        } else {
          const int total = rows_here * n;
          for (int q0 = lane; q0 < total; q0 += 64 * U) {
            T v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = src[min(q0 + 64 * u, total - 1)];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int q = q0 + 64 * u, rr = q / n;
              if (q < total) tile[rr * ldt + (q - rr * n)] = v[u];
            }
          }
        }
      } else {
        for (int q = lane; q < rows_here * w; q += 64) tile[(q / w) * ldt + (q % w)] = Wt[(base + q / w) * n + c0 + (q % w)];
      }
      wave_sync();
      if (lane < rows_here) {
        // the four basis components of a column are the same for every lane: SCALAR loads of the padded [n][4] table (a
        // lane walking its row read them as 4 LDS broadcasts per column -- 96 of the 120 LDS reads per row at 24 columns)
        const T *tr = tile + lane * ldt;
        typedef const double __attribute__((address_space(4))) *cptr_t;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
        cptr_t mcs = (cptr_t)(Mr4 + 4 * (size_t)c0);
#pragma clang diagnostic pop
        int c = 0;
        for (; c + 4 <= w; c += 4) {
          double mv[16];
#pragma unroll
          for (int e = 0; e < 16; ++e) mv[e] = mcs[4 * c + e];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const double x = (double)tr[c + u] - smu[c0 + c + u];
            acc[0] += x * mv[4 * u]; acc[1] += x * mv[4 * u + 1]; acc[2] += x * mv[4 * u + 2]; acc[3] += x * mv[4 * u + 3];
          }
        }
        for (; c < w; ++c) {
          const double x = (double)tr[c] - smu[c0 + c];
          acc[0] += x * mcs[4 * c]; acc[1] += x * mcs[4 * c + 1]; acc[2] += x * mcs[4 * c + 2]; acc[3] += x * mcs[4 * c + 3];
        }
      }
      wave_sync();
    }
    if (lane < rows_here)
      for (int i = 0; i < r; ++i) S[(size_t)i * n_rows + base + lane] = (T)acc[i];
  }
}

// ---- 64 rows per wave through LDS: the rows [base, base + rows_here) x n of a row-major matrix are one contiguous byte
// range -- moved with coalesced accesses to / from a padded LDS tile (odd stride: a lane walking its own row is
// conflict-free), so that a thread-per-row kernel neither reads nor writes memory at a row stride per lane
// (k_scale_rows as one lane per row in global memory: ~4 ms of a 10 ms depth iteration at 5 M x 24 fp64).
// (batches of eight independent loads, then their eight stores: written as one load and one store per trip the loop waited
// for every load before it issued the next -- 24 round trips for a 64 x 24 tile, and the "tiled" kernels ran at 1-2.5 TB/s)
template <typename T>
__device__ __forceinline__ void tile_load(const T *__restrict__ src, long long base, int rows_here, int n, T *tile, int ldt, int lane) {
  const T *s = src + base * n;
  const int total = rows_here * n;
  constexpr int U = 8;
  for (int q0 = lane; q0 < total; q0 += 64 * U) {
    T v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = s[min(q0 + 64 * u, total - 1)];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + 64 * u, rr = q / n;
      if (q < total) tile[rr * ldt + (q - rr * n)] = v[u];
    }
  }
}
template <typename T>
__device__ __forceinline__ void tile_store(T *__restrict__ dst, long long base, int rows_here, int n, const T *tile, int ldt, int lane) {
  T *d = dst + base * n;
  const int total = rows_here * n;
  constexpr int U = 8;
  for (int q0 = lane; q0 < total; q0 += 64 * U) {
    T v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = min(q0 + 64 * u, total - 1), rr = q / n;
      v[u] = tile[rr * ldt + (q - rr * n)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (q0 + 64 * u < total) d[q0 + 64 * u] = v[u];
  }
}

// ---- depth-weighted matrix from a resident base (mvsvd_run_scaled): W[a][j] = X[a][j] z[a][j / group] s,
// s = 1 / |row a of X o z| (norm 1: every row to unit length, ref perspective_camera_calibration.py:86-87) or
// s = 1 / sum over rows and the group's columns of (X o z)^2 (norm 2: every column group -- image -- divided by its
// SQUARED Frobenius norm, ref :170-172).  One thread per row; the group sums of norm 2 are per-block partials added in
// fixed order (k_group_scale).
template <typename T>
__global__ __launch_bounds__(256) void k_group_sumsq(const T *__restrict__ X, const T *__restrict__ z, long long n_rows, int n,
                                                     int group, double *__restrict__ part /*[gridDim.x][n / group]*/) {
  const int ng = n / group;
  // thread t of the block owns group t % ng of the rows t / ng, t / ng + rows_per_pass, ...: every group's partial is
  // accumulated by a fixed set of threads in a fixed order, then summed over those threads in thread order
  if (ng > (int)blockDim.x) {  // more groups than threads: a thread owns the groups t, t + 256, ... of the block's rows (blockIdx.x, + gridDim.x, ...)
    for (int g = threadIdx.x; g < ng; g += blockDim.x) {
      double acc = 0.0;
      for (long long a = blockIdx.x; a < n_rows; a += gridDim.x) {
        const double zz = (double)z[a * ng + g];
        for (int c = 0; c < group; ++c) {
          const double w = (double)X[a * n + g * group + c] * zz;
          acc += w * w;
        }
      }
      part[(size_t)blockIdx.x * ng + g] = acc;
    }
    return;
  }
  const int rows_per_pass = blockDim.x / ng;
  const int g = threadIdx.x % ng, rloc = threadIdx.x / ng;
  double acc = 0.0;
  if (rloc < rows_per_pass)
    for (long long a = (long long)blockIdx.x * rows_per_pass + rloc; a < n_rows; a += (long long)gridDim.x * rows_per_pass) {
      const double zz = (double)z[a * ng + g];
      for (int c = 0; c < group; ++c) {
        const double w = (double)X[a * n + g * group + c] * zz;
        acc += w * w;
      }
    }
  __shared__ double s_acc[256];
  s_acc[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < ng) {
    double t = 0.0;
    for (int r = 0; r < rows_per_pass; ++r) t += s_acc[r * ng + threadIdx.x];
    part[(size_t)blockIdx.x * ng + threadIdx.x] = t;
  }
}

// fixed-order sum of `count` values spaced `stride` apart by ONE WAVE: lane l adds the values l, l + 64, ... in order, then a
// fixed tree over the lanes (the same result whatever the launch geometry; a single thread walking 2048 partials took 0.1-0.5 ms)
__device__ __forceinline__ double wave_strided_sum(const double *__restrict__ p, int count, size_t stride, int lane) {
  double t = 0.0;
  for (int b = lane; b < count; b += 64) t += p[(size_t)b * stride];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
  return t;  // (valid in lane 0)
}

// cs[g] = 1 / (sum over the blocks, in order, of part[g * group_stride + block * block_stride]): k_group_sumsq leaves part[block][g], k_dual_apply_xz gpart[g][block]
__global__ void k_group_scale(const double *__restrict__ part, int blocks, int ng, size_t group_stride, size_t block_stride, double *__restrict__ cs) {
  const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= ng) return;
  const double t = wave_strided_sum(part + g * group_stride, blocks, block_stride, lane);
  if (lane == 0) cs[g] = 1.0 / t;
}

// mvsvd_load_images: one image's coordinates [n_rows][2] (float or double, as the caller holds them) into its two columns of the
// measurement matrix W^T [n_rows][2 m]   (ref lib/affine_camera_calibration.py:224-240: np.hstack(data_list))
template <typename S, typename T>
__global__ __launch_bounds__(256) void k_image_cols(const S *__restrict__ xy, long long n_rows, int n, int col, T *__restrict__ W) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows) return;
  T *o = W + i * n + col;
  o[0] = (T)xy[2 * i];
  o[1] = (T)xy[2 * i + 1];
}

// mvsvd_load_base_images: one image's pixel coordinates [n_rows][2] (doubles, as the caller holds them) into its three columns
// of the base, homogeneous: (x / f0, y / f0, 1)   (ref lib/perspective_camera_calibration.py:34-40)
template <typename T>
__global__ __launch_bounds__(256) void k_base_image(const double2 *__restrict__ xy, long long n_rows, int n, int col, double f0, T *__restrict__ X) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows) return;
  const double2 p = xy[i];
  T *o = X + i * n + col;
  o[0] = (T)(p.x / f0);
  o[1] = (T)(p.y / f0);
  o[2] = (T)1;
}

// Rows too long for the LDS tiles (more than ~57 fp64 / 117 fp32 columns + depths): the lanes of a wave run ACROSS the column
// groups of a row -- P = ng rounded up to a power of two lanes per row, 64 / P rows per pass (beyond 64 groups: one row, the lanes
// striding over its groups) -- so that a pass reads and writes one contiguous range; the row's sum of squares (norm 1) is a
// fixed tree over its lanes.  (Rounds 3-5 had a lane per row walking the 720 bytes of its own row here: 3.9 ms at 1 M x 90 fp64,
// more than the factorisation it feeds; this form 0.6.)
// The geometry, shared with the depth updates of the same form (k_depth_primary_wide, k_dual_apply_wide: groups = images): this
// lane is lane g0 of the P that share row rr of the R rows of a pass, and takes the row's groups g0, g0 + P, ...
struct RowLanes {
  int P = 1, R, rr, g0;
  __device__ __forceinline__ RowLanes(int groups, int lane) {
    while (P < groups && P < 64) P <<= 1;
    R = 64 / P; rr = lane / P; g0 = lane - rr * P;
  }
  template <typename... D>  // every argument summed over the row's P lanes in a fixed tree (every lane ends with the row's sums)
  __device__ __forceinline__ void sum(D &...v) const {
    for (int off = P >> 1; off > 0; off >>= 1) ((v += __shfl_xor(v, off, 64)), ...);
  }
};
template <typename T>
__global__ __launch_bounds__(256) void k_scale_rows_wide(const T *__restrict__ X, const T *__restrict__ z, long long n_rows, int n,
                                                         int group, int norm, const double *__restrict__ cs, T *__restrict__ W) {
  const int ng = n / group;
  const RowLanes L(ng, threadIdx.x & 63);
  const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * (blockDim.x >> 6);
  for (long long a0 = wave * L.R; a0 < n_rows; a0 += n_waves * L.R) {
    const long long a = a0 + L.rr;
    const bool row_ok = a < n_rows;
    double ss = 0.0;
    if (norm == 1) {
      for (int g = L.g0; g < ng; g += L.P) {
        if (row_ok) {
          const double zz = (double)z[a * ng + g];
          for (int c = 0; c < group; ++c) {
            const double w = (double)X[a * n + g * group + c] * zz;
            ss += w * w;
          }
        }
      }
      L.sum(ss);
    }
    const double rs = norm == 1 ? 1.0 / sqrt(ss) : 1.0;
    if (row_ok)
      for (int g = L.g0; g < ng; g += L.P) {
        const double f = (double)z[a * ng + g] * (norm == 2 ? cs[g] : rs);
        for (int c = 0; c < group; ++c) W[a * n + g * group + c] = (T)((double)X[a * n + g * group + c] * f);
      }
  }
}

// the same through LDS tiles (one wave = 64 rows; columns [X row | z row] side by side in the tile)
template <typename T>
__global__ __launch_bounds__(256) void k_scale_rows_tiled(const T *__restrict__ X, const T *__restrict__ z, long long n_rows, int n,
                                                          int group, int norm, const double *__restrict__ cs, T *__restrict__ W) {
  extern __shared__ double sm_raw[];
  const int ng = n / group, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ldt = (n + ng) | 1;
  T *tile = reinterpret_cast<T *>(sm_raw) + (size_t)wave * 64 * ldt;
  for (long long base = ((long long)blockIdx.x * 4 + wave) * 64; base < n_rows; base += (long long)gridDim.x * 256) {
    const int rows_here = (int)min<long long>(64, n_rows - base);
    tile_load(X, base, rows_here, n, tile, ldt, lane);
    tile_load(z, base, rows_here, ng, tile + n, ldt, lane);
    wave_sync();
    if (lane < rows_here) {
      T *xr = tile + lane * ldt;
      const T *zr = xr + n;
      double rs = 1.0;
      if (norm == 1) {
        double ss = 0.0;
        for (int g = 0; g < ng; ++g) {
          const double zz = (double)zr[g];
          for (int c = 0; c < group; ++c) {
            const double w = (double)xr[g * group + c] * zz;
            ss += w * w;
          }
        }
        rs = 1.0 / sqrt(ss);
      }
      for (int g = 0; g < ng; ++g) {
        const double f = (double)zr[g] * (norm == 2 ? cs[g] : rs);
        for (int c = 0; c < group; ++c) xr[g * group + c] = (T)((double)xr[g * group + c] * f);
      }
    }
    wave_sync();
    tile_store(W, base, rows_here, n, tile, ldt, lane);
    wave_sync();
  }
}

// sum of a value over the block's threads in a fixed tree -> part[blockIdx.x]
__device__ __forceinline__ void block_sum_to(double v, double *__restrict__ part) {
  __shared__ double s_red[256];
  s_red[threadIdx.x] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_red[threadIdx.x] += s_red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = s_red[0];
}

template <typename T>
__global__ __launch_bounds__(256) void k_fill(T *__restrict__ p, long long n, T v) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = v;
}
