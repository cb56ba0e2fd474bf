// libmvba.so -- thin SVD of a tall-skinny measurement matrix for the factorization
// initialisation (ref lib/factorization.py:5-15; inline SVD call sites
// lib/affine_camera_calibration.py:19,71,152 with the centring of :224-240).
//
// The reference calls np.linalg.svd(W) with full_matrices=True on W = (2m|3m) x N and
// keeps U[:, :r], diag(sigma[:r]) Vt[:r]; the N x N factor it discards cannot exist at
// N = 5M.  Here W^T ("Wt", N x n, row-major: exactly the array the callers hold) is
// streamed twice:
//   K7a k_gram     G = Wt^T Wt (+ column sums), fp64 accumulation whatever the input dtype
//   K7b k_jacobi   eigen-decomposition of the n x n Gram matrix, one workgroup,
//                  round-robin parallel Jacobi (n/2 independent rotations per step)
//   K7c k_project  S = M^T W, i.e. S[i][row] = sum_c M[c][i] Wt[row][c]
// sigma = sqrt(eig), M = eigenvectors of the r largest.  With fp64 accumulation the Gram
// route loses nothing for fp32 data (eps32 >> eps64 * cond^2 for the leading triplets).
// For fp64 DATA one Gram pass squares the condition number (a singular value 1e-7 below the
// largest would only be good to 1e-2), so a second, preconditioned pass follows:
//   K7d k_rotate   B = (Wt - 1 mu^T) V1            (V1 = eigenvectors of the first pass)
//   K7a again      G2 = B^T B: nearly diagonal and GRADED -- its entries are formed from B's own
//                  columns, i.e. accurate relative to the product of the two column norms, not to
//                  sigma_1^2 -- and Jacobi with the relative threshold keeps that accuracy
//   V = V1 V2, sigma = sqrt(eig G2): small singular values good to ~eps * sigma_1, like gesdd.
// Centring subtracts the column means from the rows BEFORE they enter the Gram product
// (G - s s^T / N cancels when |mean| >> spread).
// A workspace handle (mvsvd_create / load / run / destroy) keeps the matrix, every buffer, the
// stream and the events resident across calls; mvsvd_factorize is the one-shot form.
// The kernels are in the mvsvd_*.h headers included below, one per stage.  The tile sizes they share with the host (GT, GRAM_ROWS,
// WB, JW, PC, FZ_MAXM, ...) and the one formula of every kernel's dynamic LDS are in mvba_host.h, host arithmetic that host_check.cpp
// holds to the limits; the headers and the host side after them (kernel tables, step pieces, state notes) are mapped in DESIGN.md §4.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "mvba_common.h"
#include "mvba_host.h"

using namespace mvba;

namespace {

constexpr int GRAM_SLICES = 32;    // second level of the fixed-order Gram reduction
constexpr int COLSUM_SLICES = 256;
typedef double svd_d4 __attribute__((ext_vector_type(4)));

#include "mvsvd_gram.h"         // K7a / K7d: the Gram products, their fixed-order reduction, column means, rotations
#include "mvsvd_wide.h"         // n > WIDE_MIN columns: the implicit block iteration
#include "mvsvd_jacobi.h"       // K7b: the eigen-solvers
#include "mvsvd_rows.h"         // K7c and the row walkers: projection, LDS row tiles, W = X o z, fixed-order sums
#include "mvsvd_depth.h"        // the depth update: shared arithmetic, the kernels that read S from memory
#include "mvsvd_depth_fused.h"  // the depth iteration that never writes the re-weighted matrix

}  // namespace

// Workspace: the resident matrix and every buffer a factorisation needs, allocated once.
struct mvsvd_handle {
  int device = 0, dtype = 0, n = 0;
  long long max_rows = 0, n_rows = 0, base_rows = 0;  // rows of the loaded matrix (dW) / of the resident base (dX)
  hipStream_t st = nullptr;
  hipEvent_t ev[8] = {};
  DevBufs mem;  // every device buffer below (h->mem.alloc): freed by mvsvd_destroy
  void *dW = nullptr, *dS = nullptr;
  double *dG = nullptr, *dV = nullptr, *dV1 = nullptr, *dsum = nullptr, *dMr = nullptr, *dmu = nullptr, *dpart = nullptr, *dpart2 = nullptr, *dB = nullptr;
  int *dsw = nullptr;
  void *dstage = nullptr;             // mvsvd_load_images: one image's [max_rows][2] array on its way into its two columns
  void *dX = nullptr, *dz = nullptr;  // mvsvd_load_base / mvsvd_run_scaled: resident base matrix, the depths of one call
  double *dgs = nullptr;              // column-group partial sums and scales
  bool base_loaded = false;
  int depth_group = 0;                // mvsvd_depth_begin: columns per image (3); 0 = no depth loop started
  bool cs_valid = false;              // fused depth iteration: the per-image scales of norm 2 belong to the depths in dz
  double *ddep = nullptr;             // depth iteration: error partials, 12 x 12 problems, vectors (one allocation)
  size_t ddep_n = 0;                  // ... its size in doubles
  int *ddflag = nullptr;
  int chunks = 1, rank_cap = 0;
  // wide path (n > WIDE_MIN): bases Q, Z [n][WB], products B, B2 [max_rows][WB] (dBw / dB2), row-chunk partials of Z, small problems
  double *dQ = nullptr, *dZ = nullptr, *dQ2 = nullptr, *dBw = nullptr, *dB2 = nullptr, *dzpart = nullptr, *dsmall = nullptr;
  int *dwflag = nullptr;
  int zchunks = 1, wide_iters = 0;
  bool wide = false;
  bool wide_warm = false, wide_have_q = false, wide_q_center = false;  // warm start of the block iteration inside a depth loop
  long long zrows_per_chunk = 0;
  double h2d_ms = 0.0;
  bool loaded = false;
};

namespace {

// ---- kernel tables ("Map of the host side").  The only places that name an instantiation of a kernel that has
// several forms or takes more than the default LDS: the launch and set_lds_limits (mvsvd_create) both go through them.  The
// dynamic LDS of a launch is its kernel's one formula in mvba_host.h, where the limit it is raised to stands beside it.
template <typename T>
auto gram_fused_kernel(int mode) { return mode == 1 ? k_gram_fused<T, 1> : (mode == 2 ? k_gram_fused<T, 2> : k_gram_fused<T, 3>); }
// the fused depth iteration's Gram pass: m images (2, 4, .. FZ_MAXM), the norm of the depth method, with or without the rotation by V1
template <int M>
auto gram_xz_kernel_m(int norm, bool rot) {
  if (norm == 1) return rot ? k_gram_xz<M, 1, true> : k_gram_xz<M, 1, false>;
  return rot ? k_gram_xz<M, 2, true> : k_gram_xz<M, 2, false>;
}
auto gram_xz_kernel(int m, int norm, bool rot) {
  switch (m) {
    case 2: return gram_xz_kernel_m<2>(norm, rot);
    case 4: return gram_xz_kernel_m<4>(norm, rot);
    case 6: return gram_xz_kernel_m<6>(norm, rot);
    case 8: return gram_xz_kernel_m<8>(norm, rot);
    default: return gram_xz_kernel_m<10>(norm, rot);
  }
}
auto dual_gram_mfma_kernel(int m) {
  return m == 2 ? k_dual_gram_mfma<2> : (m == 4 ? k_dual_gram_mfma<4> : (m == 6 ? k_dual_gram_mfma<6> : (m == 8 ? k_dual_gram_mfma<8> : k_dual_gram_mfma<10>)));
}
auto jacobi_kernel(int n) { return n <= JW ? k_jacobi_small : (n <= JACOBI_LDS_ORDER ? k_jacobi<true> : k_jacobi<false>); }
template <typename T>
auto rotate_rows_kernel() { return k_rotate_rows<T>; }
template <typename T>
auto project_kernel() { return k_project<T>; }
// tiled: the rows go through LDS tiles (tile_fits / depth_tiled)
template <typename T>
auto scale_rows_kernel(bool tiled) { return tiled ? k_scale_rows_tiled<T> : k_scale_rows_wide<T>; }
template <typename T>
auto depth_primary_kernel(bool tiled) { return tiled ? k_depth_primary<T> : k_depth_primary_wide<T>; }
template <typename T>
auto dual_apply_kernel(bool tiled) { return tiled ? k_dual_apply<T> : k_dual_apply_wide<T>; }
template <typename T>
auto dual_gram_kernel() { return k_dual_gram<T>; }
auto primary_xz_kernel() { return k_primary_xz; }
auto dual_apply_xz_kernel() { return k_dual_apply_xz; }

// the tail of every Gram form: the chunks' partial tiles summed in fixed order, then the full symmetric n x n matrix G
void gram_reduce_finish(mvsvd_handle *h, int n, int chunks, double *G) {
  const int n_pairs = gram_pairs(n), slices = std::min(chunks, GRAM_SLICES);
  hipLaunchKernelGGL(k_gram_reduce, dim3(n_pairs, slices), dim3(256), 0, h->st, h->dpart, chunks, n_pairs, h->dpart2);
  hipLaunchKernelGGL(k_gram_finish, dim3((n + 127) / 128, n), dim3(128), 0, h->st, h->dpart2, slices, n_pairs, gram_tiles(n), gram_mode(n) == 2 ? 1 : 0, G, n);
}
// G = (W - mu)^T (W - mu) of an n_rows x n matrix through the workspace's partial buffers (the workspace's own matrix, or -- the
// wide path -- one of its n x 32 / N x 32 blocks)
template <typename T>
void launch_gram_n(mvsvd_handle *h, const T *W, long long n_rows, int n, const double *mu, int chunks, double *G) {
  if (const int mode = gram_mode(n))
    hipLaunchKernelGGL(gram_fused_kernel<T>(mode), dim3(1, chunks), dim3(256), gram_fused_lds(sizeof(T), n), h->st, W, n_rows, n, mu, h->dpart);
  else
    hipLaunchKernelGGL(k_gram_pair<T>, dim3(gram_pairs(n), chunks), dim3(256), 0, h->st, W, n_rows, n, gram_tiles(n), gram_pairs(n), mu, h->dpart);
  gram_reduce_finish(h, n, chunks, G);
}
// ... of the resident base re-weighted by the depths in dz (and, rot, rotated by dV1), which never leaves the LDS: m = n / 3 images
void launch_gram_xz(mvsvd_handle *h, int norm, bool rot, int chunks, const double *cs) {
  const int n = h->n, m = n / 3;
  hipLaunchKernelGGL(gram_xz_kernel(m, norm, rot), dim3(1, chunks), dim3(256), gram_xz_lds(m, rot), h->st, (const double *)h->dX, (const double *)h->dz,
                     h->base_rows, n, m, cs, rot ? (const double *)h->dV1 : (const double *)nullptr, h->dpart);
  gram_reduce_finish(h, n, chunks, h->dG);
}

// `count` problems of order n (one workgroup each; more than one: n <= JW), the sweeps of the last pass -> *sweeps.
// tol: rotate while |a_pq| > tol sqrt(|a_pp a_qq|).  1e-15 for float64 input; float32 input carries
// 6e-8 of relative noise per entry, so its Gram matrix is diagonalised to 1e-11 (one or two sweeps fewer).
void launch_jacobi_n(mvsvd_handle *h, double *dA, int n, double *dVout, double tol, int count, int *sweeps) {
  const int np = (n + 1) & ~1;
  const int threads = n <= JW ? JHB * JHB + JW * (np / 2) /* A blocks + V pieces */ : (n <= JACOBI_LDS_ORDER ? 256 : 1024);
  hipLaunchKernelGGL(jacobi_kernel(n), dim3(count), dim3(threads), jacobi_lds(n), h->st, dA, dVout, n, 60, tol, sweeps);
}
void launch_jacobi(mvsvd_handle *h, double *dVout, double tol) { launch_jacobi_n(h, h->dG, h->n, dVout, tol, 1, h->dsw); }

// B = (W - 1 mu^T) V, V n x n: in 64 x 64 tiles, or -- tall and narrow -- streamed GRAM_ROWS rows at a time
template <typename T>
void launch_rotate(mvsvd_handle *h, const T *W, long long n_rows, int n, const double *mu, const double *V, double *B) {
  hipLaunchKernelGGL(k_rotate<T>, dim3((unsigned)((n_rows + 63) / 64), (n + 63) / 64), dim3(256), 0, h->st, W, n_rows, n, mu, V, B);
}
template <typename T>
void launch_rotate_rows(mvsvd_handle *h, const T *W, long long n_rows, int n, const double *mu, const double *V, double *B) {
  const int grid = (int)std::max<long long>(1, std::min<long long>(6 * 256, (n_rows + GRAM_ROWS - 1) / GRAM_ROWS));
  hipLaunchKernelGGL(rotate_rows_kernel<T>(), dim3(grid), dim3(256), rotate_rows_lds(sizeof(T), n), h->st, W, n_rows, n, mu, V, B);
}

int chunks_for(long long n_rows, int n) {
  const int n_tiles = (n + GT - 1) / GT, n_pairs = n_tiles * (n_tiles + 1) / 2;
  return (int)std::max<long long>(1, std::min<long long>((n_rows + 4 * ROWS_PER_STEP - 1) / (4 * ROWS_PER_STEP),
                                                         n_tiles <= 2 ? 2048 : std::max(8, 4096 / n_pairs)));
}

// f(T()) with T the workspace's element type (or that of a caller's array)
template <typename F>
auto with_dtype(int dtype, F &&f) { return dtype == 0 ? f(float()) : f(double()); }
size_t el_bytes(const mvsvd_handle *h) { return h->dtype ? 8 : 4; }

// Device memory.  mvsvd_create allocates what every factorisation needs; the rest exists from its first use on (what is resident
// when is part of the interface: a workspace that never takes a base pays for none).  A fixed-size buffer goes through alloc_once,
// its size written once, below; the two that grow (dS with rank_cap, ddep with ddep_n) through regrow, which leaves a null pointer
// and capacity 0 behind a failed allocation, so that the next call allocates again instead of launching onto the freed buffer.
template <typename P>
int alloc_once(mvsvd_handle *h, P *&p, size_t bytes) { return p ? MVBA_OK : h->mem.alloc((char **)&p, bytes); }
template <typename P, typename C>
int regrow(mvsvd_handle *h, P *&p, C &cap, C want, size_t bytes) {
  if (cap >= want) return MVBA_OK;
  MVBA_HIP(hipStreamSynchronize(h->st));
  h->mem.release(p);
  cap = 0;
  if (int rc = h->mem.alloc((char **)&p, bytes)) return rc;
  cap = want;
  return MVBA_OK;
}
int need_refine_b(mvsvd_handle *h) { return alloc_once(h, h->dB, sizeof(double) * (size_t)h->max_rows * h->n); }
int need_stage(mvsvd_handle *h) { return alloc_once(h, h->dstage, 16 * (size_t)h->max_rows); }
int need_base(mvsvd_handle *h) { return alloc_once(h, h->dX, el_bytes(h) * (size_t)h->max_rows * h->n); }
int need_depths(mvsvd_handle *h) { return alloc_once(h, h->dz, el_bytes(h) * (size_t)h->max_rows * h->n); }  // (room for any grouping: a later call may ask for a finer one)
int need_depth_flags(mvsvd_handle *h) { return alloc_once(h, h->ddflag, sizeof(int) * (size_t)(h->n / 3 + 1)); }
int need_rank(mvsvd_handle *h, int n_rank) { return regrow(h, h->dS, h->rank_cap, n_rank, el_bytes(h) * (size_t)h->max_rows * n_rank); }
constexpr int GS_BLOCKS = 512;
// dgs: the column groups' partial sums [GS_BLOCKS][gs_stride], and behind them their scales -> *cs
int group_scales(mvsvd_handle *h, double **cs) {
  const size_t gs_stride = (size_t)std::max(256, h->n);  // (room for the finest grouping: one group per column)
  if (int rc = alloc_once(h, h->dgs, sizeof(double) * (size_t)(GS_BLOCKS + 1) * gs_stride)) return rc;
  *cs = h->dgs + (size_t)GS_BLOCKS * gs_stride;
  return MVBA_OK;
}

// timings[0 .. 5] of a call from its events: slot s is ev[p[s][0]] .. ev[p[s][1]] in ms, 0 where the caller names no pair (-1).
// What a slot means is the interface's (include/mvba.h); which pass of a route goes into it is the caller's to say.
double event_ms(mvsvd_handle *h, int a, int b) {
  float ms = 0.f;
  if (a >= 0) hipEventElapsedTime(&ms, h->ev[a], h->ev[b]);
  return ms;
}
void read_timings(mvsvd_handle *h, double *timings, const int (&p)[6][2]) {
  for (int s = 0; s < 6; ++s) timings[s] = event_ms(h, p[s][0], p[s][1]);
}
double jacobi_sweeps(mvsvd_handle *h) {  // of the last pass
  int sw = 0;
  hipMemcpy(&sw, h->dsw, sizeof(int), hipMemcpyDeviceToHost);
  return sw;
}

// What the workspace holds, in one place each.  dW: a matrix a factorisation may run on (`loaded`); dX: the base of the depth
// loops; depth_group / cs_valid: a depth loop and its norm-2 scales, which belong to one base; wide_warm / wide_have_q: the block
// iteration may start from the previous factorisation's vectors, which holds only between re-weightings of one base.
void matrix_replaced(mvsvd_handle *h, long long n_rows) {  // mvsvd_load, mvsvd_load_images
  h->n_rows = n_rows;
  h->loaded = true;
  h->wide_warm = h->wide_have_q = false;  // a new matrix: the block iteration starts from its fixed block
}
void base_replaced(mvsvd_handle *h, long long n_rows) {  // mvsvd_load_base, mvsvd_load_base_images
  h->base_rows = n_rows;
  h->base_loaded = true;
  h->depth_group = 0;  // a new base ends a depth loop: its depths and norm-2 scales belong to the old one
  h->cs_valid = false;
  h->wide_warm = h->wide_have_q = false;
  h->loaded = false;  // dW holds nothing derived from this base yet (or was the staging buffer)
}
void base_scaled_into_w(mvsvd_handle *h) {  // scale_base_into_w
  h->n_rows = h->base_rows;  // dW now holds the re-weighted base (a mvsvd_load in between may have changed n_rows)
  h->loaded = true;
  h->wide_warm = true;  // (the block iteration may start from the previous factorisation's vectors: the same base, other depths)
}

// ---- step pieces, each written once
// the column means of the loaded matrix -> dmu: the rows are centred as they enter the products.  Null without centring.
template <typename T>
const double *column_means(mvsvd_handle *h, int center) {
  if (!center) return nullptr;
  const int n = h->n, cy = (int)std::max<long long>(1, std::min<long long>(COLSUM_SLICES, h->n_rows / 4096));
  hipLaunchKernelGGL(k_colsum<T>, dim3(n, cy), dim3(256), 0, h->st, (const T *)h->dW, h->n_rows, n, h->dsum);
  hipLaunchKernelGGL(k_mean_from_sum, dim3((n + 255) / 256), dim3(256), 0, h->st, h->dsum, cy, n, h->n_rows, h->dmu);
  return h->dmu;
}
// the second, preconditioned pass on the Gram matrix of B = W V1 in dG: V2 (into dMr, n x n: sized for it), then V = V1 V2
void second_jacobi(mvsvd_handle *h) {
  launch_jacobi(h, h->dMr, 1e-15);
  launch_rotate<double>(h, h->dV1, (long long)h->n, h->n, nullptr, h->dMr, h->dV);
}
// A diagonalised k x k matrix (dD: eigenvalues on its diagonal) and its n x k vectors (dV) -> host, with the means if asked for;
// sort, the rank-r basis with a deterministic sign.  k = n after the Jacobi route, WB after the block iteration.
struct HostBasis {
  std::vector<double> D, V, mu;
  Basis basis;
};
int read_basis(mvsvd_handle *h, const double *dD, const double *dV, int k, int n_rank, bool means, HostBasis &b) {
  const int n = h->n;
  b.D.resize((size_t)k * k);
  b.V.resize((size_t)n * k);
  b.mu.assign(n, 0.0);
  MVBA_HIP(hipMemcpyAsync(b.D.data(), dD, sizeof(double) * b.D.size(), hipMemcpyDeviceToHost, h->st));
  MVBA_HIP(hipMemcpyAsync(b.V.data(), dV, sizeof(double) * b.V.size(), hipMemcpyDeviceToHost, h->st));
  if (means) MVBA_HIP(hipMemcpyAsync(b.mu.data(), h->dmu, sizeof(double) * n, hipMemcpyDeviceToHost, h->st));
  MVBA_HIP(hipStreamSynchronize(h->st));
  return select_basis(b.D.data(), b.V.data(), k, n, n_rank, b.basis);
}
// ... handed to the caller: sigma (NaN beyond the k computed), M [n][n_rank], the means
template <typename T>
void write_basis(const HostBasis &b, int k, int n, int n_rank, T *sigma, T *M, T *means) {
  for (int i = 0; i < n; ++i) sigma[i] = i < k ? (T)std::sqrt(std::max(0.0, b.D[(size_t)b.basis.order[i] * k + b.basis.order[i]])) : (T)NAN;
  for (int i = 0; i < n_rank; ++i)
    for (int c = 0; c < n; ++c) M[(size_t)c * n_rank + i] = (T)basis_at(b.basis, b.V.data(), k, c, i);
  if (means)
    for (int c = 0; c < n; ++c) means[c] = (T)b.mu[c];
}

template <typename T>
int run_wide(mvsvd_handle *h, int n_rank, int center, T *M, T *sigma, T *S, T *means, double *timings);

template <typename T>
int run(mvsvd_handle *h, int n_rank, int center, T *M, T *sigma, T *S, T *means, double *timings) {
  if (wide_route(h->wide, h->n, n_rank)) return run_wide<T>(h, n_rank, center, M, sigma, S, means, timings);
  const int n = h->n;
  const long long n_rows = h->n_rows;
  hipStream_t st = h->st;
  const T *dW = (const T *)h->dW;
  const int chunks = chunks_for(n_rows, n);
  const bool refine = sizeof(T) == 8;  // fp64 data: second, preconditioned pass (see the file header)
  hipEventRecord(h->ev[1], st);
  const double *mu = column_means<T>(h, center);
  launch_gram_n<T>(h, dW, n_rows, n, mu, chunks, h->dG);
  hipEventRecord(h->ev[2], st);
  launch_jacobi(h, refine ? h->dV1 : h->dV, sizeof(T) == 8 ? 1e-15 : 1e-11);
  hipEventRecord(h->ev[3], st);
  if (refine) {
    if (int rc = need_refine_b(h)) return rc;
    if (rotate_streams(sizeof(T), n_rows, n))  // tall and narrow: the streaming form
      launch_rotate_rows<T>(h, dW, n_rows, n, mu, h->dV1, h->dB);
    else
      launch_rotate<T>(h, dW, n_rows, n, mu, h->dV1, h->dB);
    launch_gram_n<double>(h, h->dB, n_rows, n, nullptr, chunks, h->dG);
    second_jacobi(h);
  }
  HostBasis b;
  if (int rc = read_basis(h, h->dG, h->dV, n, n_rank, center != 0, b)) return rc;
  write_basis<T>(b, n, n, n_rank, sigma, M, means);
  // S = M^T W in groups of (up to) 4 basis vectors per pass over W
  if (int rc = need_rank(h, n_rank)) return rc;
  hipEventRecord(h->ev[4], st);
  const int pgrid = (int)std::max<long long>(1, std::min<long long>(4096, (n_rows + 255) / 256));
  std::vector<double> Mg((size_t)n * 4);
  for (int g0 = 0; g0 < n_rank; g0 += 4) {
    const int rg = std::min(4, n_rank - g0);
    basis_block(b.basis, b.V.data(), n, n, g0, n_rank, Mg.data());
    MVBA_HIP(hipMemcpyAsync(h->dMr, Mg.data(), sizeof(double) * (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(project_kernel<T>(), dim3(pgrid), dim3(256), project_lds(sizeof(T), n), st, dW, n_rows, n, rg, h->dMr, mu, (T *)h->dS + (size_t)g0 * n_rows);
    MVBA_HIP(hipStreamSynchronize(st));  // Mg is reused by the next group
  }
  hipEventRecord(h->ev[5], st);
  if (S) MVBA_HIP(hipMemcpyAsync(S, h->dS, sizeof(T) * (size_t)n_rows * n_rank, hipMemcpyDeviceToHost, st));  // (null: S stays on the device)
  MVBA_HIP(hipStreamSynchronize(st));
  MVBA_HIP(hipGetLastError());
  if (timings) {  // means + Gram | Jacobi (first pass) | projection | refinement pass (rotate, Gram, Jacobi, V1 V2)
    read_timings(h, timings, {{-1, -1}, {1, 2}, {2, 3}, {4, 5}, {-1, -1}, {refine ? 3 : -1, 4}});
    timings[0] = h->h2d_ms;  // H2D of the last load
    timings[4] = jacobi_sweeps(h);
  }
  return MVBA_OK;
}

// The factorisation of a wide matrix (n > WIDE_MIN columns): block power iteration with Rayleigh-Ritz, see the kernels' header.
template <typename T>
int run_wide(mvsvd_handle *h, int n_rank, int center, T *M, T *sigma, T *S, T *means, double *timings) {
  const int n = h->n;
  const long long N = h->n_rows;
  hipStream_t st = h->st;
  const T *dW = (const T *)h->dW;
  if (n_rank > WB / 2)
    return fail(MVBA_ERR_BADARG, "n_cols > " + std::to_string(JACOBI_MAX) + ": the block iteration carries " + std::to_string(WB) + " vectors, n_rank <= " + std::to_string(WB / 2));
  hipEventRecord(h->ev[1], st);
  const double *mu = column_means<T>(h, center);
  hipEventRecord(h->ev[2], st);
  double *H = h->dsmall, *Y = H + WB * WB, *C = Y + WB * WB, *V = C + WB * WB, *Tm = V + WB * WB, *dres = Tm + WB * WB, *respart = dres + WB;
  int *dcol = h->dwflag + WB;                      // [WB] columns to take at the end
  double *dsgn = respart + (size_t)WB * ((n + 255) / 256);  // [WB] their signs
  const int chunksB = chunks_for(N, WB), chunksZ = chunks_for(n, WB);
  const int wgrid = (int)((N + WT - 1) / WT), ngrid = (int)(((long long)n * WB + 255) / 256), rgrid = (n + 255) / 256;
  auto orth = [&](double *src, double *tmp, double *dst, const double *ritz, unsigned long long salt) {  // dst <- orthonormal basis of span(src), in Ritz order; src and tmp are scratch
    launch_gram_n<double>(h, src, n, WB, nullptr, chunksZ, C);
    hipLaunchKernelGGL(k_chol_orth, dim3(1), dim3(64), 0, st, C, ritz, Tm, h->dwflag);
    launch_rotate_rows<double>(h, src, n, WB, nullptr, Tm, tmp);
    hipLaunchKernelGGL(k_wide_refill, dim3(ngrid), dim3(256), 0, st, tmp, n, h->dwflag, salt);
    launch_gram_n<double>(h, tmp, n, WB, nullptr, chunksZ, C);
    hipLaunchKernelGGL(k_chol_orth, dim3(1), dim3(64), 0, st, C, (const double *)nullptr, Tm, h->dwflag);
    launch_rotate_rows<double>(h, tmp, n, WB, nullptr, Tm, dst);
  };
  auto product_b = [&](const double *Q) {  // B = (W - mu) Q, H = B^T B, Jacobi: theta on H's diagonal, Y
    hipLaunchKernelGGL(k_wq<T>, dim3(wgrid), dim3(256), 0, st, dW, N, n, mu, Q, h->dBw);
    launch_gram_n<double>(h, h->dBw, N, WB, nullptr, chunksB, H);
    launch_jacobi_n(h, H, WB, Y, 1e-15, 1, h->dsw);
  };
  // start: a fixed pseudo-random block, orthonormalised -- or, inside a depth loop (the same base re-weighted by slightly different
  // depths, 50-200 times: mvsvd_run_scaled / mvsvd_depth_step), the Ritz vectors the previous factorisation ended with: one or two
  // iterations instead of three or four.  A newly loaded matrix (mvsvd_load / mvsvd_load_base) always starts from the fixed block.
  if (!(h->wide_warm && h->wide_have_q && h->wide_q_center == (center != 0))) {
    hipLaunchKernelGGL(k_wide_init, dim3(ngrid), dim3(256), 0, st, h->dZ, n, 0x5eedull);
    orth(h->dZ, h->dQ2, h->dQ, nullptr, 1);
  }
  h->wide_have_q = false;  // (until this call has converged)
  double theta[WB], res[WB];
  const int max_iter = 2000;
  int it = 0;
  // Residuals of the leading n_rank Ritz pairs (k_ritz: the part of W^T W q_j outside the block): `worst` relative to theta_1 (what
  // the leading triplets need: <= 1e-13, or at this matrix's rounding floor -- no halving over three iterations -- below 1e-10)
  // and `rel`, each against its own pair's scale max(1e-12 theta_j, 50 eps sqrt(theta_1 theta_j)): the angle of a SMALL
  // triplet's vector is r_j / theta_j (a sigma_4 = 1e-7 sigma_1 is invisible at the 1e-13 theta_1 level), and
  // eps sigma_1 / sigma_j is what the products W q, W^T b leave of it.
  double worst = 0.0, rel = 0.0, best = 1e300, best_rel = 1e300;
  int stalled = 0, stalled_rel = 0;
  bool converged = false;
  for (; it < max_iter; ++it) {
    product_b(h->dQ);
    launch_rotate_rows<double>(h, h->dBw, N, WB, nullptr, Y, h->dB2);  // B Y = W (Q Y)
    hipLaunchKernelGGL(k_wtb<T>, dim3((n + WT - 1) / WT, h->zchunks), dim3(256), 0, st, dW, N, n, mu, h->dB2, h->zrows_per_chunk, h->dzpart);
    hipLaunchKernelGGL(k_sum_chunks, dim3(ngrid), dim3(256), 0, st, h->dzpart, h->zchunks, (long long)n * WB, h->dZ);
    hipLaunchKernelGGL(k_ritz, dim3(rgrid), dim3(256), 0, st, h->dQ, (const double *)h->dZ, n, Y, H, respart);
    hipLaunchKernelGGL(k_sum_chunks, dim3(1), dim3(256), 0, st, respart, rgrid, (long long)WB, dres);
    std::vector<double> hH((size_t)WB * WB);
    MVBA_HIP(hipMemcpyAsync(hH.data(), H, sizeof(double) * WB * WB, hipMemcpyDeviceToHost, st));
    MVBA_HIP(hipMemcpyAsync(res, dres, sizeof(double) * WB, hipMemcpyDeviceToHost, st));
    MVBA_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < WB; ++j) {
      theta[j] = hH[(size_t)j * WB + j];
      if (!std::isfinite(theta[j]) || !std::isfinite(res[j]))  // (before anything is compared: max() and sort() swallow a NaN)
        return fail(MVBA_ERR_SINGULAR, "SVD did not converge (non-finite values in the measurement matrix)");
    }
    int order[WB];
    descending_order(theta, 1, WB, order);
    const double tmax = std::max(theta[order[0]], 0.0);
    worst = rel = 0.0;
    for (int i = 0; i < n_rank; ++i) {
      const double rj = std::sqrt(std::max(res[order[i]], 0.0)), tj = theta[order[i]];
      worst = std::max(worst, rj);
      if (tj > 1e-28 * tmax) rel = std::max(rel, rj / std::max(1e-12 * tj, 1.1e-14 * std::sqrt(tmax * tj)));  // (sigma_j below 1e-14 sigma_1 is numerically zero: the absolute measure covers it)
    }
    worst = tmax > 0.0 ? worst / tmax : 0.0;
    if (!(worst == worst) || !(rel == rel)) return fail(MVBA_ERR_SINGULAR, "SVD did not converge (non-finite values in the measurement matrix)");
    if (worst < 0.5 * best) { best = worst; stalled = 0; } else ++stalled;
    if (rel < 0.5 * best_rel) { best_rel = rel; stalled_rel = 0; } else ++stalled_rel;
    const bool done_abs = worst <= 1e-13 || (stalled >= 3 && worst <= 1e-10), done_rel = rel <= 1.0 || stalled_rel >= 3;
    if (done_abs && done_rel) { converged = true; ++it; break; }
    orth(h->dZ, h->dQ2, h->dQ, H, 2 + (unsigned long long)it);
  }
  h->wide_iters = it;
  h->wide_have_q = converged;
  h->wide_q_center = center != 0;
  if (!converged)
    return fail(MVBA_ERR_SINGULAR, "SVD did not converge: block power iteration, residual " + std::to_string(worst) + " of sigma_1^2 after " + std::to_string(it) +
                                       " iterations (singular values " + std::to_string(n_rank) + " .. " + std::to_string(WB) + " of this matrix are too close)");
  hipEventRecord(h->ev[3], st);
  // final pass: Q holds the Ritz vectors; B = (W - mu) Q has a nearly diagonal, graded Gram matrix -> sigma and the last rotation
  product_b(h->dQ);
  hipLaunchKernelGGL(k_ritz, dim3(rgrid), dim3(256), 0, st, h->dQ, (const double *)nullptr, n, Y, H, (double *)nullptr);
  launch_rotate_rows<double>(h, h->dBw, N, WB, nullptr, Y, h->dB2);
  HostBasis b;
  if (int rc = read_basis(h, H, h->dQ, WB, n_rank, center != 0, b)) return rc;
  write_basis<T>(b, WB, n, n_rank, sigma, M, means);
  int hcol[WB] = {};
  double hsgn[WB] = {};
  std::copy_n(b.basis.order.begin(), n_rank, hcol);
  std::copy_n(b.basis.sign.begin(), n_rank, hsgn);
  if (int rc = need_rank(h, n_rank)) return rc;
  hipEventRecord(h->ev[4], st);
  std::vector<double> Mg((size_t)n * 4);  // the depth loops read the leading basis vectors as [n][4] from dMr, like after run()
  basis_block(b.basis, b.V.data(), WB, n, 0, n_rank, Mg.data());
  MVBA_HIP(hipMemcpyAsync(h->dMr, Mg.data(), sizeof(double) * (size_t)n * 4, hipMemcpyHostToDevice, st));
  MVBA_HIP(hipMemcpyAsync(dcol, hcol, sizeof(int) * WB, hipMemcpyHostToDevice, st));
  MVBA_HIP(hipMemcpyAsync(dsgn, hsgn, sizeof(double) * WB, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_take_cols<T>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, h->dB2, N, n_rank, dcol, dsgn, (T *)h->dS);
  hipEventRecord(h->ev[5], st);
  if (S) MVBA_HIP(hipMemcpyAsync(S, h->dS, sizeof(T) * (size_t)N * n_rank, hipMemcpyDeviceToHost, st));  // (null: S stays on the device)
  MVBA_HIP(hipStreamSynchronize(st));  // (hcol / hsgn are read by the copies above)
  MVBA_HIP(hipGetLastError());
  if (timings) {  // means | the iteration (in the eigen-solver's slot) | S out of B | final pass
    read_timings(h, timings, {{-1, -1}, {1, 2}, {2, 3}, {4, 5}, {-1, -1}, {3, 4}});
    timings[0] = h->h2d_ms;
    timings[4] = it;  // iterations (in the sweeps' slot)
  }
  return MVBA_OK;
}

// cs[g] <- 1 / the squared norm of column group g of the base re-weighted by the depths in dz (norm 2), through dgs
template <typename T>
void launch_group_scales(mvsvd_handle *h, int group, double *cs) {
  const int ng = h->n / group, gblocks = (int)std::max<long long>(1, std::min<long long>(GS_BLOCKS, h->base_rows / 64 + 1));
  hipLaunchKernelGGL(k_group_sumsq<T>, dim3(gblocks), dim3(256), 0, h->st, (const T *)h->dX, (const T *)h->dz, h->base_rows, h->n, group, h->dgs);
  hipLaunchKernelGGL(k_group_scale, dim3((ng + 3) / 4), dim3(256), 0, h->st, h->dgs, gblocks, ng, (size_t)1, (size_t)ng, cs);  // dgs[block][group]
}

// dW <- the resident base re-weighted by the depths in dz and normalised (see mvsvd_run_scaled)
int scale_base_into_w(mvsvd_handle *h, int group, int norm) {
  const int cols = h->n + h->n / group;  // a row's values and its depths
  double *cs;
  if (int rc = group_scales(h, &cs)) return rc;
  const int sgrid = (int)std::max<long long>(1, std::min<long long>(4096, (h->base_rows + 255) / 256));
  with_dtype(h->dtype, [&](auto tag) {
    using T = decltype(tag);
    if (norm == 2) launch_group_scales<T>(h, group, cs);
    const bool tiled = tile_fits(sizeof(T), cols);
    hipLaunchKernelGGL(scale_rows_kernel<T>(tiled), dim3(sgrid), dim3(256), tiled ? row_tile_lds(sizeof(T), cols) : 0, h->st, (const T *)h->dX, (const T *)h->dz,
                       h->base_rows, h->n, group, norm, cs, (T *)h->dW);
  });
  MVBA_HIP(hipGetLastError());
  base_scaled_into_w(h);
  return MVBA_OK;
}

constexpr int DEPTH_BLOCKS = 2048;  // blocks of the per-point passes / of the dual Gram pass
inline int depth_grid(long long rows) { return (int)std::max<long long>(1, std::min<long long>(DEPTH_BLOCKS, (rows + 255) / 256)); }

// The depth iteration's scratch (ddep: DepthScratch) with `own` doubles behind the common part, and the dual method's flags.  The
// two routes differ in `own` and one handle may take both (a new base on the other side of the fused route's row threshold,
// MVSVD_DEPTH_UNFUSED read per call): ddep grows to the larger.
int depth_scratch(mvsvd_handle *h, size_t own, DepthScratch *out) {
  const int m = h->n / 3;
  const size_t need = DepthScratch::prefix(DEPTH_BLOCKS, m) + own;
  if (int rc = regrow(h, h->ddep, h->ddep_n, need, sizeof(double) * need)) return rc;
  if (int rc = need_depth_flags(h)) return rc;
  *out = DepthScratch(h->ddep, DEPTH_BLOCKS, m);
  return MVBA_OK;
}

// is[i] = 1 / sigma_i of the leading four, which the dual method divides by: all of them must be positive
int inverse_sigmas(const double (&sigma)[4], double (&is)[4]) {
  for (int i = 0; i < 4; ++i) {
    if (!(sigma[i] > 0.0)) return fail(MVBA_ERR_SINGULAR, "measurement matrix has rank < 4");
    is[i] = 1.0 / sigma[i];
  }
  return MVBA_OK;
}
// The dual method's companion problems, from the `parts` partials per entry in d.own (mfma: in k_dual_gram_mfma's layout): their
// sums in order -> G12, colsum; Jacobi on the m problems of order 12 -> V12; the images' vectors -> w12 (ddflag[0], cleared by the caller: set where an image has none)
void dual_companion(mvsvd_handle *h, const DepthScratch &d, int m, bool mfma, int parts) {
  if (mfma)
    hipLaunchKernelGGL(k_dual_reduce_mfma, dim3((m * 90 + 3) / 4), dim3(256), 0, h->st, d.own, parts, m, d.G12, d.colsum);
  else
    hipLaunchKernelGGL(k_dual_reduce, dim3((14 * m * 6 + 3) / 4), dim3(256), 0, h->st, d.own, parts, m, d.G12, d.colsum);
  launch_jacobi_n(h, d.G12, 12, d.V12, 1e-15, m, h->ddflag + 1);
  hipLaunchKernelGGL(k_dual_vec, dim3((m + 63) / 64), dim3(64), 0, h->st, d.G12, d.V12, d.colsum, m, d.w12, h->ddflag);
}
// the end of a depth step: the error of the update from its `blocks` partials -> *E, event 7, the dual method's flag
int finish_depth_step(mvsvd_handle *h, const DepthScratch &d, int blocks, int method, double f0, double *E) {
  hipStream_t st = h->st;
  hipLaunchKernelGGL(k_depth_error, dim3(1), dim3(64), 0, st, d.Epart, blocks, (double)h->base_rows * (double)(h->n / 3), f0, d.Eout);
  hipEventRecord(h->ev[7], st);
  MVBA_HIP(hipGetLastError());
  int fl = 0;
  MVBA_HIP(hipMemcpyAsync(E, d.Eout, sizeof(double), hipMemcpyDeviceToHost, st));
  if (method == 2) MVBA_HIP(hipMemcpyAsync(&fl, h->ddflag, sizeof(int), hipMemcpyDeviceToHost, st));
  MVBA_HIP(hipStreamSynchronize(st));
  if (fl) return fail(MVBA_ERR_SINGULAR, "depth iteration: an image's 12 x 12 companion matrix has no positive eigenvalue");
  return MVBA_OK;
}

// A depth step: factorise the base re-weighted by the depths in dz, update the depths by the method, finish.  This form factorises
// through dW (any dtype, any image count up to DEPTH_MAX_IMAGES) ...
template <typename T>
int depth_step(mvsvd_handle *h, int method, double f0, double *E, double *timings) {
  const int n = h->n, m = n / 3;
  const long long rows = h->base_rows;
  int rc = scale_base_into_w(h, 3, method);
  if (rc) return rc;
  std::vector<T> M((size_t)n * 4), sigma(n);
  rc = run<T>(h, 4, 0, M.data(), sigma.data(), (T *)nullptr, (T *)nullptr, timings);  // dMr = M, dS = S stay on the device
  if (rc) return rc;
  const int dsplit = dual_gram_split(m);  // thread groups of k_dual_gram, each with its own partial
  const int dual_blocks = std::max(64, std::min(DEPTH_BLOCKS, 95000 / m / dsplit));  // (blocks x groups partials of 14 m x 6 doubles: <= ~64 MB)
  const long long rpb = (rows + dual_blocks - 1) / dual_blocks;
  const int gblocks = (int)((rows + rpb - 1) / rpb);
  DepthScratch d;
  if ((rc = depth_scratch(h, (size_t)dual_blocks * dsplit * 14 * m * 6, &d))) return rc;  // (own: the dual partials)
  const int pgrid = depth_grid(rows);
  const bool tiled = depth_tiled(sizeof(T), m);
  const T *dX = (const T *)h->dX, *dS = (const T *)h->dS;
  hipStream_t st = h->st;
  hipEventRecord(h->ev[6], st);
  if (method == 1) {
    hipLaunchKernelGGL(depth_primary_kernel<T>(tiled), dim3(pgrid), dim3(256), tiled ? depth_primary_lds(sizeof(T), m) : depth_primary_wide_lds(m), st, dX, h->dMr, dS,
                       rows, m, (T *)h->dz, d.Epart);
  } else {
    double is[4];
    if ((rc = inverse_sigmas({(double)sigma[0], (double)sigma[1], (double)sigma[2], (double)sigma[3]}, is))) return rc;
    MVBA_HIP(hipMemsetAsync(h->ddflag, 0, sizeof(int), st));
    const int dg_rows = dual_gram_rows(m);  // (128 up to 47 images, 24 at 256: the launch used to FAIL from 48 images on)
    hipLaunchKernelGGL(dual_gram_kernel<T>(), dim3(gblocks), dim3(256), dual_gram_lds(m, dg_rows), st, dX, dS, is[0], is[1], is[2], is[3], rows, m, rpb, dg_rows, d.own);
    dual_companion(h, d, m, false, gblocks * dsplit);
    hipLaunchKernelGGL(dual_apply_kernel<T>(tiled), dim3(pgrid), dim3(256), tiled ? dual_apply_lds(sizeof(T), m) : dual_apply_wide_lds(m), st, dX, dS,
                       is[0], is[1], is[2], is[3], h->dMr, d.w12, rows, m, (T *)h->dz, d.Epart);
  }
  if ((rc = finish_depth_step(h, d, pgrid, method, f0, E))) return rc;
  if (timings) timings[0] = event_ms(h, 6, 7);  // (no upload in a depth step: slot 0 carries the depth-update kernels instead)
  return MVBA_OK;
}

// ... and this one never writes the re-weighted matrix (see k_gram_xz): fp64, n = 3 m <= 32 columns, n even.
bool fused_depth_ok(const mvsvd_handle *h) {
  return h->dtype == 1 && h->n <= 32 && h->n % 2 == 0 && h->n / 3 <= FZ_MAXM && h->base_rows >= 256 && !getenv("MVSVD_DEPTH_UNFUSED");
}
int depth_step_fused(mvsvd_handle *h, int method, double f0, double *E, double *timings) {
  const int n = h->n, m = n / 3;
  const long long rows = h->base_rows;
  hipStream_t st = h->st;
  const double *dX = (const double *)h->dX;
  double *dz = (double *)h->dz;
  double *cs;
  if (int rc = group_scales(h, &cs)) return rc;
  const size_t dual_part = (size_t)512 * 4 * m * 256;  // k_dual_gram_mfma: a 16 x 16 tile per wave and image, at most 512 workgroups
  DepthScratch d;
  if (int rc = depth_scratch(h, dual_part + (size_t)FZ_MAXM * DEPTH_BLOCKS, &d)) return rc;
  double *gsum = d.own + dual_part;  // (own: the dual partials, then the images' sums of the next scales)
  if (method == 2 && !h->cs_valid) {  // the per-image scales of the depths the loop holds (first dual step, or after primary steps)
    launch_group_scales<double>(h, 3, cs);
    h->cs_valid = true;
  }
  const int chunks = chunks_for(rows, n);
  hipEventRecord(h->ev[1], st);
  launch_gram_xz(h, method, false, chunks, cs);
  hipEventRecord(h->ev[2], st);
  launch_jacobi(h, h->dV1, 1e-15);
  hipEventRecord(h->ev[3], st);
  launch_gram_xz(h, method, true, chunks, cs);  // B = W V1 never leaves the LDS
  second_jacobi(h);
  hipEventRecord(h->ev[4], st);
  HostBasis b;
  if (int rc = read_basis(h, h->dG, h->dV, n, 4, false, b)) return rc;
  std::vector<double> Mg((size_t)n * 4);
  double sigma[4], is[4];
  for (int i = 0; i < 4; ++i) sigma[i] = std::sqrt(std::max(0.0, b.D[(size_t)b.basis.order[i] * n + b.basis.order[i]]));
  if (method == 2)
    if (int rc = inverse_sigmas(sigma, is)) return rc;
  basis_block(b.basis, b.V.data(), n, n, 0, 4, Mg.data());
  MVBA_HIP(hipMemcpyAsync(h->dMr, Mg.data(), sizeof(double) * (size_t)n * 4, hipMemcpyHostToDevice, st));
  const int pgrid = depth_grid(rows);
  hipEventRecord(h->ev[6], st);
  if (method == 1) {
    hipLaunchKernelGGL(primary_xz_kernel(), dim3(pgrid), dim3(256), depth_primary_lds(sizeof(double), m), st, dX, h->dMr, rows, m, dz, d.Epart);
    h->cs_valid = false;
  } else {
    MVBA_HIP(hipMemsetAsync(h->ddflag, 0, sizeof(int), st));
    const int mblocks = (int)std::max<long long>(1, std::min<long long>(512, (rows + GRAM_ROWS - 1) / GRAM_ROWS));  // two workgroups per CU
    hipLaunchKernelGGL(dual_gram_mfma_kernel(m), dim3(mblocks), dim3(256), dual_gram_mfma_lds(m), st, dX, (const double *)dz, cs, h->dMr, is[0], is[1], is[2], is[3], rows,
                       m, d.own);
    dual_companion(h, d, m, true, mblocks * 4);
    hipLaunchKernelGGL(dual_apply_xz_kernel(), dim3(pgrid), dim3(256), dual_apply_lds(sizeof(double), m), st, dX, cs, is[0], is[1], is[2], is[3], h->dMr, d.w12, rows, m,
                       dz, d.Epart, gsum);
    hipLaunchKernelGGL(k_group_scale, dim3((m + 3) / 4), dim3(256), 0, st, gsum, pgrid, m, (size_t)pgrid, (size_t)1, cs);  // gsum[image][block]: the next iteration's scales
  }
  const int rc = finish_depth_step(h, d, pgrid, method, f0, E);
  h->loaded = false;  // (no re-weighted matrix was written: dW holds nothing that belongs to these depths)
  if (rc) return rc;
  if (timings) {  // depth update | first Gram pass | Jacobi (first pass) | (no projection pass) | refinement pass (rotate + Gram fused, Jacobi, V1 V2)
    read_timings(h, timings, {{6, 7}, {1, 2}, {2, 3}, {-1, -1}, {-1, -1}, {3, 4}});
    timings[4] = jacobi_sweeps(h);
  }
  return MVBA_OK;
}

// mvsvd_create: every kernel that may ask for more than LDS_DEFAULT is raised to its limit (mvba_host.h), by walking the tables
int set_lds_limits() {
  auto raise = [](auto kernel, size_t limit) { return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit); };
  MVBA_HIP(raise(jacobi_kernel(JACOBI_LDS_ORDER), JACOBI_LDS_MAX));
  MVBA_HIP(raise(primary_xz_kernel(), DEPTH_LDS_MAX));
  MVBA_HIP(raise(dual_apply_xz_kernel(), DEPTH_LDS_MAX));
  for (int m = 2; m <= FZ_MAXM; m += 2) {
    MVBA_HIP(raise(dual_gram_mfma_kernel(m), DEPTH_LDS_MAX));
    for (int norm : {1, 2})
      for (bool rot : {false, true}) MVBA_HIP(raise(gram_xz_kernel(m, norm, rot), DEPTH_LDS_MAX));
  }
  for (int dtype : {0, 1})
    if (int rc = with_dtype(dtype, [&](auto tag) -> int {
          using T = decltype(tag);
          MVBA_HIP(raise(rotate_rows_kernel<T>(), ROTATE_LDS_MAX));
          MVBA_HIP(raise(project_kernel<T>(), PROJECT_LDS_MAX));
          MVBA_HIP(raise(scale_rows_kernel<T>(true), DEPTH_LDS_MAX));  // (the other form takes no dynamic LDS)
          MVBA_HIP(raise(dual_gram_kernel<T>(), DEPTH_LDS_MAX));
          for (bool tiled : {false, true}) {
            MVBA_HIP(raise(depth_primary_kernel<T>(tiled), DEPTH_LDS_MAX));
            MVBA_HIP(raise(dual_apply_kernel<T>(tiled), DEPTH_LDS_MAX));
          }
          return MVBA_OK;
        }))
      return rc;
  return MVBA_OK;
}

// mvsvd_create's work on a fresh handle.  Returns at the first failure: the caller destroys the handle, whatever it holds by then.
int create_workspace(mvsvd_handle *h, int64_t max_rows, int32_t n_cols, int32_t dtype) {
  MVBA_HIP(hipGetDevice(&h->device));
  h->dtype = dtype; h->n = n_cols; h->max_rows = max_rows;
  const bool wide = n_cols > WIDE_MIN, dense = n_cols <= JACOBI_MAX;  // beyond JACOBI_MAX no n x n matrix at all: see run_wide
  h->wide = wide;
  const size_t el = dtype ? 8 : 4, nn = dense ? (size_t)n_cols * n_cols : (size_t)WB * WB;
  const int gram_n = dense ? n_cols : WB;  // the Gram kernels run on the workspace's matrix and on the wide path's 32-column blocks
  const int n_pairs = gram_tiles(gram_n) * (gram_tiles(gram_n) + 1) / 2;
  h->chunks = chunks_for(max_rows, gram_n);
  // partial tiles of the Gram kernels: the workspace's own matrix and / or the wide path's blocks (N x 32 and n x 32: three tile pairs)
  size_t part_tiles = (size_t)h->chunks * n_pairs, part2_tiles = (size_t)GRAM_SLICES * n_pairs;
  if (wide) {
    part_tiles = std::max(part_tiles, (size_t)3 * std::max(chunks_for(max_rows, WB), chunks_for(n_cols, WB)));
    part2_tiles = std::max(part2_tiles, (size_t)3 * GRAM_SLICES);
  }
  MVBA_HIP(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
  for (auto &e : h->ev) MVBA_HIP(hipEventCreate(&e));
  int rc = alloc_once(h, h->dW, el * (size_t)max_rows * n_cols);
  auto alloc = [&](auto *&p, size_t count) { if (!rc) rc = h->mem.alloc(&p, count); };  // (nothing more after the first failure)
  alloc(h->dG, nn);
  alloc(h->dV, nn);
  alloc(h->dV1, nn);
  alloc(h->dMr, std::max(nn, (size_t)4 * n_cols));
  alloc(h->dsum, (size_t)n_cols * COLSUM_SLICES);
  alloc(h->dmu, n_cols);
  alloc(h->dsw, 1);
  alloc(h->dpart, part_tiles * 256);
  alloc(h->dpart2, part2_tiles * 256);
  if (wide) {
    const size_t nb = (size_t)n_cols * WB;
    // row chunks of Z = W^T B: enough workgroups for the chip beside the n / 64 column blocks, a multiple of 64 rows each
    const long long col_blocks = (n_cols + WT - 1) / WT, want = std::max<long long>(1, 2048 / col_blocks);
    h->zrows_per_chunk = std::max<long long>(WT, ((max_rows + want - 1) / want + WT - 1) / WT * WT);
    h->zchunks = (int)((max_rows + h->zrows_per_chunk - 1) / h->zrows_per_chunk);
    alloc(h->dQ, nb);
    alloc(h->dZ, nb);
    alloc(h->dQ2, nb);
    alloc(h->dBw, (size_t)max_rows * WB);
    alloc(h->dB2, (size_t)max_rows * WB);
    alloc(h->dzpart, (size_t)h->zchunks * nb);
    alloc(h->dsmall, (size_t)5 * WB * WB + 2 * WB + (size_t)WB * ((n_cols + 255) / 256));
    alloc(h->dwflag, 2 * WB);
  }
  if (rc) return rc;
  return set_lds_limits();
}

// run() on the caller's arrays of the workspace's dtype
int run_any(mvsvd_handle *h, int n_rank, int center, void *M, void *sigma, void *S, void *means, double *timings) {
  return with_dtype(h->dtype, [&](auto tag) {
    using T = decltype(tag);
    return run<T>(h, n_rank, center, (T *)M, (T *)sigma, (T *)S, (T *)means, timings);
  });
}
// argument checks the entry points share
int check_rows(const mvsvd_handle *h, int64_t n_rows) {
  return n_rows < 1 || n_rows > h->max_rows ? fail(MVBA_ERR_BADARG, "n_rows outside the workspace (1 .. max_rows)") : MVBA_OK;
}
int check_images(const void *const *xy, int n_images) {
  for (int k = 0; k < n_images; ++k)
    if (!xy[k]) return fail(MVBA_ERR_BADARG, "null image array");
  return MVBA_OK;
}

}  // namespace

extern "C" {

int mvsvd_create(int64_t max_rows, int32_t n_cols, int32_t dtype, int32_t device, mvsvd_handle **out) {
  if (!out) return fail(MVBA_ERR_BADARG, "null argument");
  if (max_rows < 1 || n_cols < 1 || n_cols > MVSVD_MAX_COLS)
    return fail(MVBA_ERR_BADARG, "need max_rows >= 1 and 1 <= n_cols <= " + std::to_string(MVSVD_MAX_COLS) + " (three rows of W per image at the engine's camera limit)");
  if (dtype != 0 && dtype != 1) return fail(MVBA_ERR_BADARG, "dtype must be 0 (float32) or 1 (float64)");
  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  mvsvd_handle *h = new mvsvd_handle();
  if (int rc = create_workspace(h, max_rows, n_cols, dtype)) {
    mvsvd_destroy(h);
    return rc;
  }
  *out = h;
  return MVBA_OK;
}

void mvsvd_destroy(mvsvd_handle *h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->st) hipStreamSynchronize(h->st);
  h->mem.release_all();
  for (auto &e : h->ev)
    if (e) hipEventDestroy(e);
  if (h->st) hipStreamDestroy(h->st);
  delete h;
}

int mvsvd_load(mvsvd_handle *h, const void *Wt, int64_t n_rows) {
  if (!h || !Wt) return fail(MVBA_ERR_BADARG, "null argument");
  if (int rc = check_rows(h, n_rows)) return rc;
  MVBA_HIP(hipSetDevice(h->device));
  hipEventRecord(h->ev[0], h->st);
  MVBA_HIP(hipMemcpyAsync(h->dW, Wt, el_bytes(h) * (size_t)n_rows * h->n, hipMemcpyHostToDevice, h->st));
  hipEventRecord(h->ev[1], h->st);
  MVBA_HIP(hipStreamSynchronize(h->st));
  h->h2d_ms = event_ms(h, 0, 1);
  matrix_replaced(h, n_rows);
  return MVBA_OK;
}

int mvsvd_load_images(mvsvd_handle *h, const void *const *xy, int32_t n_images, int64_t n_rows, int32_t src_dtype) {
  if (!h || !xy) return fail(MVBA_ERR_BADARG, "null argument");
  if (int rc = check_rows(h, n_rows)) return rc;
  if (n_images < 1 || 2 * (long long)n_images != h->n) return fail(MVBA_ERR_BADARG, "the workspace must have 2 columns per image");
  if (src_dtype != 0 && src_dtype != 1) return fail(MVBA_ERR_BADARG, "src_dtype must be 0 (float32) or 1 (float64)");
  if (int rc = check_images(xy, n_images)) return rc;
  MVBA_HIP(hipSetDevice(h->device));
  if (int rc = need_stage(h)) return rc;
  const size_t bytes = (src_dtype ? 16 : 8) * (size_t)n_rows;
  const unsigned grid = (unsigned)((n_rows + 255) / 256);
  hipEventRecord(h->ev[0], h->st);
  for (int k = 0; k < n_images; ++k) {  // image after image in stream order through the one staging buffer
    MVBA_HIP(hipMemcpyAsync(h->dstage, xy[k], bytes, hipMemcpyHostToDevice, h->st));
    with_dtype(src_dtype, [&](auto src) {
      with_dtype(h->dtype, [&](auto dst) {
        using S = decltype(src);
        using T = decltype(dst);
        hipLaunchKernelGGL((k_image_cols<S, T>), dim3(grid), dim3(256), 0, h->st, (const S *)h->dstage, (long long)n_rows, h->n, 2 * k, (T *)h->dW);
      });
    });
  }
  hipEventRecord(h->ev[1], h->st);
  MVBA_HIP(hipGetLastError());
  MVBA_HIP(hipStreamSynchronize(h->st));
  h->h2d_ms = event_ms(h, 0, 1);
  matrix_replaced(h, n_rows);
  return MVBA_OK;
}

int mvsvd_run(mvsvd_handle *h, int32_t n_rank, int32_t center, void *M, void *sigma, void *S, void *means, double *timings_ms) {
  if (!h || !M || !sigma || !S) return fail(MVBA_ERR_BADARG, "null argument");
  if (!h->loaded) return fail(MVBA_ERR_STATE, "mvsvd_run before mvsvd_load");
  if (n_rank < 1 || n_rank > h->n) return fail(MVBA_ERR_BADARG, "need 1 <= n_rank <= n_cols");
  MVBA_HIP(hipSetDevice(h->device));
  return run_any(h, n_rank, center, M, sigma, S, means, timings_ms);
}

int mvsvd_load_base(mvsvd_handle *h, const void *X, int64_t n_rows) {
  if (!h || !X) return fail(MVBA_ERR_BADARG, "null argument");
  if (int rc = check_rows(h, n_rows)) return rc;
  MVBA_HIP(hipSetDevice(h->device));
  if (int rc = need_base(h)) return rc;
  MVBA_HIP(hipMemcpyAsync(h->dX, X, el_bytes(h) * (size_t)n_rows * h->n, hipMemcpyHostToDevice, h->st));
  MVBA_HIP(hipStreamSynchronize(h->st));
  base_replaced(h, n_rows);
  return MVBA_OK;
}

int mvsvd_load_base_images(mvsvd_handle *h, const double *const *xy, int32_t n_images, int64_t n_rows, double f0) {
  if (!h || !xy) return fail(MVBA_ERR_BADARG, "null argument");
  if (int rc = check_rows(h, n_rows)) return rc;
  if (n_images < 1 || 3 * (long long)n_images != h->n) return fail(MVBA_ERR_BADARG, "the workspace must have 3 columns per image");
  if (!(f0 != 0.0) || !std::isfinite(f0)) return fail(MVBA_ERR_BADARG, "f0 must be finite and non-zero");
  if (int rc = check_images((const void *const *)xy, n_images)) return rc;
  MVBA_HIP(hipSetDevice(h->device));
  if (int rc = need_base(h)) return rc;
  // staged through dW (16 bytes a row <= el * n: there are at least 6 columns), image after image in stream order
  if (el_bytes(h) * (size_t)h->n < 16) return fail(MVBA_ERR_BADARG, "the workspace is too narrow to stage an image");
  const unsigned grid = (unsigned)((n_rows + 255) / 256);
  for (int k = 0; k < n_images; ++k) {
    MVBA_HIP(hipMemcpyAsync(h->dW, xy[k], 16 * (size_t)n_rows, hipMemcpyHostToDevice, h->st));
    with_dtype(h->dtype, [&](auto tag) {
      using T = decltype(tag);
      hipLaunchKernelGGL(k_base_image<T>, dim3(grid), dim3(256), 0, h->st, (const double2 *)h->dW, (long long)n_rows, h->n, 3 * k, f0, (T *)h->dX);
    });
  }
  MVBA_HIP(hipGetLastError());
  MVBA_HIP(hipStreamSynchronize(h->st));
  base_replaced(h, n_rows);
  return MVBA_OK;
}

int mvsvd_run_scaled(mvsvd_handle *h, const void *z, int32_t group, int32_t norm, int32_t n_rank, void *M, void *sigma, void *S,
                     double *timings_ms) {
  if (!h || !M || !sigma || !S) return fail(MVBA_ERR_BADARG, "null argument");
  if (!h->base_loaded) return fail(MVBA_ERR_STATE, "mvsvd_run_scaled before mvsvd_load_base");
  // z == NULL: the depths a device depth loop left in the workspace (same grouping) -- nothing is uploaded at all
  if (!z && (h->depth_group != group || !h->dz)) return fail(MVBA_ERR_STATE, "mvsvd_run_scaled without depths: no device depth loop of this grouping has run");
  if (group < 1 || h->n % group) return fail(MVBA_ERR_BADARG, "group must divide n_cols");
  if (norm < 0 || norm > 2) return fail(MVBA_ERR_BADARG, "norm must be 0 (none), 1 (unit rows) or 2 (column groups by their squared norm)");
  if (n_rank < 1 || n_rank > h->n) return fail(MVBA_ERR_BADARG, "need 1 <= n_rank <= n_cols");
  const int ng = h->n / group;
  MVBA_HIP(hipSetDevice(h->device));
  if (int rc = need_depths(h)) return rc;
  hipEventRecord(h->ev[0], h->st);
  if (z) MVBA_HIP(hipMemcpyAsync(h->dz, z, el_bytes(h) * (size_t)h->base_rows * ng, hipMemcpyHostToDevice, h->st));  // the only upload of the call
  hipEventRecord(h->ev[1], h->st);
  if (z) h->depth_group = 0;  // (the caller's depths replace whatever a depth loop held)
  int rc = scale_base_into_w(h, group, norm);
  if (rc) return rc;
  MVBA_HIP(hipStreamSynchronize(h->st));
  h->h2d_ms = event_ms(h, 0, 1);
  return run_any(h, n_rank, 0, M, sigma, S, nullptr, timings_ms);
}

int mvsvd_depth_begin(mvsvd_handle *h, int32_t group) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  if (!h->base_loaded) return fail(MVBA_ERR_STATE, "mvsvd_depth_begin before mvsvd_load_base");
  if (group != 3 || h->n % 3) return fail(MVBA_ERR_BADARG, "the depth iteration works on homogeneous image coordinates: group = 3, n_cols = 3 m");
  if (h->n / 3 > DEPTH_MAX_IMAGES) return fail(MVBA_ERR_BADARG, "at most " + std::to_string(DEPTH_MAX_IMAGES) + " images in the device depth loop (two 12-double tables per image in a workgroup's LDS)");
  MVBA_HIP(hipSetDevice(h->device));
  const int ng = h->n / 3;
  if (int rc = need_depths(h)) return rc;  // (shared with mvsvd_run_scaled, whose groups may be finer)
  const long long cnt = h->base_rows * ng;
  const int grid = (int)std::max<long long>(1, std::min<long long>(4096, (cnt + 255) / 256));
  with_dtype(h->dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(k_fill<T>, dim3(grid), dim3(256), 0, h->st, (T *)h->dz, cnt, (T)1);
  });
  MVBA_HIP(hipGetLastError());
  h->depth_group = 3;
  h->cs_valid = false;
  return MVBA_OK;
}

int mvsvd_depth_step(mvsvd_handle *h, int32_t method, double f0, double *E, double *timings_ms) {
  if (!h || !E) return fail(MVBA_ERR_BADARG, "null argument");
  if (!h->base_loaded || h->depth_group != 3) return fail(MVBA_ERR_STATE, "mvsvd_depth_step before mvsvd_depth_begin");
  if (method != 1 && method != 2) return fail(MVBA_ERR_BADARG, "method must be 1 (primary) or 2 (dual)");
  if (h->n < 6) return fail(MVBA_ERR_BADARG, "the rank-4 depth iteration needs at least 2 images (3 m >= 4 columns, as the reference's)");
  MVBA_HIP(hipSetDevice(h->device));
  if (fused_depth_ok(h)) return depth_step_fused(h, method, f0, E, timings_ms);
  h->cs_valid = false;  // (the unfused route moves the depths without the fused route's norm-2 scales)
  return with_dtype(h->dtype, [&](auto tag) { return depth_step<decltype(tag)>(h, method, f0, E, timings_ms); });
}

int mvsvd_depth_read(mvsvd_handle *h, void *z) {
  if (!h || !z) return fail(MVBA_ERR_BADARG, "null argument");
  if (!h->base_loaded || h->depth_group != 3) return fail(MVBA_ERR_STATE, "mvsvd_depth_read before mvsvd_depth_begin");
  MVBA_HIP(hipSetDevice(h->device));
  MVBA_HIP(hipMemcpyAsync(z, h->dz, el_bytes(h) * (size_t)h->base_rows * (h->n / 3), hipMemcpyDeviceToHost, h->st));
  MVBA_HIP(hipStreamSynchronize(h->st));
  return MVBA_OK;
}

int mvsvd_factorize(const void *Wt, int64_t n_rows, int32_t n_cols, int32_t dtype, int32_t n_rank, int32_t center, void *M,
                    void *sigma, void *S, void *means, double *timings_ms, int32_t device) {
  if (!Wt || !M || !sigma || !S) return fail(MVBA_ERR_BADARG, "null argument");
  if (n_rows < 1 || n_cols < 1 || n_rank < 1 || n_rank > n_cols) return fail(MVBA_ERR_BADARG, "need n_rows >= 1, 1 <= n_rank <= n_cols");
  mvsvd_handle *h = nullptr;
  int rc = mvsvd_create(n_rows, n_cols, dtype, device, &h);
  if (rc) return rc;
  rc = mvsvd_load(h, Wt, n_rows);
  if (!rc) rc = mvsvd_run(h, n_rank, center, M, sigma, S, means, timings_ms);
  mvsvd_destroy(h);
  return rc;
}

}  // extern "C"
