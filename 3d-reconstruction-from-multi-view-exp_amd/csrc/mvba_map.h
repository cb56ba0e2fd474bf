// Parameter maps (mvba_set_parameter_map) -- kernels, gfx950.
//
// Included by mvba.hip inside its device-code namespace, after mvba_cov.h: uses NB, packed_sym, tri_tile, keep_index, sig_block.
// Nothing here runs while the engine has the default map.
//
// A map sends parameter slot g = 9 k + p to a reduced unknown col[g] in [0, D') or holds it (-1); slots with the same
// unknown are tied.  With P[g][col g] = 1 the trial solves (P^T A P) x = P^T b, dxi = P x, on the packed [A | b] that K3 and
// the all-reduce leave.  The device tables are the map itself and its transpose in CSR form:
//   col [9m]                      unknown of every slot, or -1
//   mptr [D' + 1], mem [n_mapped]  the slots of every unknown, ascending
// and U, the number of leading unknowns with exactly one slot (the Python layer orders the untied unknowns first, so U is
// all of them; any other order is solved as well, only more of it through the row kernel below).
//   k_map_compact      the U x U corner of the lower triangle: k_compact's transposing gather with a table in keep_index's place;
//                      the right-hand-side row (sums over the members) and the back-substitution's progress words
//   k_map_rows         rows U .. D'-1: M[i][j] = sum over members(i) x members(j) of A[g][g'], a row's members dealt to four
//                      slices of a workgroup, the slices added in a fixed order -- except where row AND column are tied:
//   k_map_tied         a tied x tied entry is a sum of members(i) x members(j) terms (m^2 for a parameter shared by all cameras):
//                      several workgroups per entry, each a share of the row's members against all of the column's (read along a
//                      packed row), a fixed-tree block sum into a partial; k_map_tied_finish adds an entry's partials in order
//   k_map_full         the same sums into the LU rescue's full augmented matrix (tied x tied entries again by k_map_tied)
//   k_map_expand       dxi[g] = x[col g], 0 where held
//   k_map_cov_expand   Cov = P Sigma' P^T into the camera-block table, one thread per table entry
// No atomics on floating-point data: every sum has a fixed order, two runs are bitwise equal.

// One workgroup per 32 x 32 tile of the lower triangle of the untied corner (nt = ceil(U / 32) tile rows), then one per 256
// columns of the right-hand-side row.  As k_compact: the packed rows are read along their length and written through a
// transposing LDS tile.
__global__ __launch_bounds__(256) void k_map_compact(int D, int ld, int m, int U, int nt, const double *__restrict__ Afull,
                                                     const double *__restrict__ bfull, const int *__restrict__ mptr,
                                                     const int *__restrict__ mem, double *__restrict__ M, unsigned *__restrict__ bar,
                                                     int nsync) {
  __shared__ double tile[NB][NB + 1];
  const int ntri = nt * (nt + 1) / 2, t = blockIdx.x, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  if (t >= ntri) {
    const int j = (t - ntri) * 256 + threadIdx.x;
    if (j < nsync) bar[j] = 0u;
    if (j < D) {
      double s = bfull[mem[mptr[j]]];
      for (int q = mptr[j] + 1; q < mptr[j + 1]; ++q) s += bfull[mem[q]];
      M[(size_t)D * ld + j] = s;
    }
    return;
  }
  int I, J;
  tri_tile(t, I, J);
  const int gi = mem[mptr[min(NB * I + tx, U - 1)]];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int gj = mem[mptr[min(NB * J + ty + 8 * q, U - 1)]];
    tile[ty + 8 * q][tx] = packed_sym(Afull, m, gi, gj);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = NB * I + ty + 8 * q, j = NB * J + tx;
    if (i < U && j <= i) M[(size_t)i * ld + j] = tile[tx][ty + 8 * q];
  }
}

// Row i = U + blockIdx.y, columns 64 blockIdx.x .. + 63 (those <= i).  Thread (cj, s): column j = 64 blockIdx.x + cj, members
// s, s + 4, ... of the row, all members of the column.  For members above the column's slot the loads of a wave run along a
// packed row (consecutive columns are consecutive slots); for those below it they walk down a packed column, where the three
// rows of a shared (f, u, v) meet the same lines in L2.
__global__ __launch_bounds__(256) void k_map_rows(int D, int ld, int m, int U, const double *__restrict__ Afull,
                                                  const int *__restrict__ mptr, const int *__restrict__ mem, double *__restrict__ M) {
  __shared__ double part[4][64];
  const int i = U + blockIdx.y, cj = threadIdx.x & 63, s = threadIdx.x >> 6, j = 64 * blockIdx.x + cj;
  if (64 * (int)blockIdx.x > i) return;  // (uniform)
  double acc = 0.0;
  const int q0 = mptr[i], q1 = mptr[i + 1];
  bool mine = j <= i;  // (a tied x tied entry belongs to k_map_tied)
  if (mine) {
    const int p0 = mptr[j], p1 = mptr[j + 1];
    mine = q1 - q0 == 1 || p1 - p0 == 1;
    if (mine)
    for (int q = q0 + s; q < q1; q += 4) {
      const int g = mem[q];
      for (int p = p0; p < p1; ++p) acc += packed_sym(Afull, m, g, mem[p]);
    }
  }
  part[s][cj] = acc;
  __syncthreads();
  if (s == 0 && mine) M[(size_t)i * ld + j] = (part[0][cj] + part[1][cj]) + (part[2][cj] + part[3][cj]);
}

// Tied x tied entries, listed by the host as pairs (i, j <= i) of tied unknowns.  blockIdx.x: the pair; blockIdx.y: the share of
// the row's members (y, y + gridDim.y, ...); the threads run over the column's members -- slots 9 cameras apart in the packed
// row of the row's slot, wherever that slot is the smaller one.  part[pair][share] = the block's sum (block_sum: a fixed tree).
__global__ __launch_bounds__(256) void k_map_tied(int m, const double *__restrict__ Afull, const int *__restrict__ mptr,
                                                  const int *__restrict__ mem, const int2 *__restrict__ pairs,
                                                  double *__restrict__ part) {
  __shared__ double s_red[16];
  const int2 pr = pairs[blockIdx.x];
  const int q0 = mptr[pr.x], nq = mptr[pr.x + 1] - q0, p0 = mptr[pr.y], np = mptr[pr.y + 1] - p0;
  double acc = 0.0;
  for (int q = blockIdx.y; q < nq; q += gridDim.y) {
    const int g = mem[q0 + q];
    for (int p = threadIdx.x; p < np; p += 256) acc += packed_sym(Afull, m, g, mem[p0 + p]);
  }
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) part[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = t;
}

// One thread per pair: its partials in order, into M[i][j] (row stride ld); `mirror`: the LU rescue's full matrix, both triangles.
__global__ __launch_bounds__(256) void k_map_tied_finish(int n_pairs, int nblk, int ld, int mirror, const int2 *__restrict__ pairs,
                                                         const double *__restrict__ part, double *__restrict__ M) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_pairs) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(size_t)e * nblk + b];
  const int2 pr = pairs[e];
  M[(size_t)pr.x * ld + pr.y] = s;
  if (mirror) M[(size_t)pr.y * ld + pr.x] = s;
}

// LU rescue: the full D' x (D' + 1) augmented matrix [P^T A P | P^T b], one thread per entry (rare path)
__global__ void k_map_full(int D, int m, const double *__restrict__ Apk, const double *__restrict__ bfull,
                           const int *__restrict__ mptr, const int *__restrict__ mem, double *__restrict__ F) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;  // j in [0, D]: column D is the right-hand side
  if (j > D) return;
  double acc = 0.0;
  if (j < D && mptr[i + 1] - mptr[i] > 1 && mptr[j + 1] - mptr[j] > 1) return;  // tied x tied: k_map_tied
  for (int q = mptr[i]; q < mptr[i + 1]; ++q) {
    const int g = mem[q];
    if (j == D) { acc += bfull[g]; continue; }
    for (int p = mptr[j]; p < mptr[j + 1]; ++p) acc += packed_sym(Apk, m, g, mem[p]);
  }
  F[(size_t)i * (D + 1) + j] = acc;
}

// The back-substitution kernels scatter x through keep_index (into `xs`, a scratch vector): unknown j sits at keep_index(j).
__global__ __launch_bounds__(256) void k_map_expand(int n9, int gauge_axis, const int *__restrict__ col,
                                                    const double *__restrict__ xs, double *__restrict__ dxi) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n9) return;
  const int j = col[g];
  dxi[g] = j < 0 ? 0.0 : xs[keep_index(j, gauge_axis)];
}

// k_cov_lauum has scattered Sigma' = (P^T S P)^-1 through keep_index into a table `sigv` of mv camera blocks per side; entry
// (g, g') of block (k, l >= k) of the real table is Sigma'[col g][col g'], 0 where either is held.  blockIdx.y = k.
__global__ __launch_bounds__(256) void k_map_cov_expand(int m, int mv, int gauge_axis, const int *__restrict__ col,
                                                        const double *__restrict__ sigv, double *__restrict__ sig) {
  const int k = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 81 * (m - k)) return;
  const int l = k + t / 81, a = t % 81, j1 = col[9 * k + a / 9], j2 = col[9 * l + a % 9];
  double v = 0.0;
  if (j1 >= 0 && j2 >= 0) {
    const int g1 = keep_index(min(j1, j2), gauge_axis), g2 = keep_index(max(j1, j2), gauge_axis), k1 = g1 / 9, k2 = g2 / 9;
    v = sigv[sig_block(k1, k2, mv) + 9 * (g1 - 9 * k1) + (g2 - 9 * k2)];
  }
  sig[sig_block(k, l, m) + a] = v;
}
