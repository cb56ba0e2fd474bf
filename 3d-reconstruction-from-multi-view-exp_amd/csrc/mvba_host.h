// Host-side helpers for libmvba.so: what mvba.hip (the bundle-adjustment engine) and mvsvd.hip (the SVD workspace) share, and the
// pure host pieces of the SVD workspace (no HIP call in them: csrc/host_check.cpp runs them under the host sanitizers).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <numeric>
#include <vector>

#include "mvba_common.h"

namespace mvba {

// Device buffers with one owner.  Whatever alloc() hands out is freed when the owner goes: a DevBufs on the stack holds the
// temporaries of one call (every early return frees them), the one inside mvba_handle holds the engine's buffers (mvba_destroy
// frees them all: a new member of mvba_handle needs no second edit).  release() frees one buffer early; adopt() moves one over
// from another owner.
struct DevBufs {
  std::vector<void *> bufs;
  DevBufs() = default;
  DevBufs(const DevBufs &) = delete;
  DevBufs &operator=(const DevBufs &) = delete;
  ~DevBufs() { release_all(); }
  template <typename T>
  int alloc(T **p, size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    const hipError_t e = hipMalloc((void **)p, bytes);
    if (e != hipSuccess) {  // say how much was asked for and how much there is: "out of memory" alone does not tell a scene from a knob
      size_t fr = 0, tot = 0;
      hipMemGetInfo(&fr, &tot);
      *p = nullptr;
      return fail(MVBA_ERR_HIP, std::string("hipMalloc of ") + std::to_string(bytes) + " bytes: " + hipGetErrorString(e) + " (" + std::to_string(fr >> 20) +
                                    " MiB free of " + std::to_string(tot >> 20) + ")");
    }
    bufs.push_back(*p);
    return MVBA_OK;
  }
  void own(void *q) { bufs.push_back(q); }  // a buffer the caller allocated itself
  bool forget(void *q) {
    auto it = std::find(bufs.begin(), bufs.end(), q);
    if (it == bufs.end()) return false;
    bufs.erase(it);
    return true;
  }
  template <typename T>
  void release(T *&p) {
    if (p && forget(p)) hipFree(p);
    p = nullptr;
  }
  template <typename T>
  void adopt(DevBufs &from, T *p) {
    if (p && from.forget(p)) bufs.push_back(p);
  }
  void release_all() {
    for (void *q : bufs) hipFree(q);
    bufs.clear();
  }
};

// ------------------------------------------------------------------ SVD workspace, host arithmetic only
// order[0 .. k) <- the indices of v[0], v[stride], ..., v[(k - 1) stride], largest value first
inline void descending_order(const double *v, size_t stride, int k, int *order) {
  std::iota(order, order + k, 0);
  std::sort(order, order + k, [&](int a, int b) { return v[(size_t)a * stride] > v[(size_t)b * stride]; });
}

// The basis a factorisation hands out, chosen from a diagonalised k x k matrix D (eigenvalues on its diagonal) and the n x k matrix
// V of the vectors that belong to them (row-major, leading dimension k): `order` lists all k eigenvalues, largest first, and
// sign[i] makes the largest-magnitude component of vector order[i] positive (the first such index on ties) for i < n_rank.
struct Basis {
  std::vector<int> order;
  std::vector<double> sign;
};
inline int select_basis(const double *D, const double *V, int k, int n, int n_rank, Basis &b) {
  for (int i = 0; i < k; ++i)  // (np.linalg.svd raises LinAlgError("SVD did not converge") on such input; max() and sort() below would swallow the NaN)
    if (!std::isfinite(D[(size_t)i * k + i])) return fail(MVBA_ERR_SINGULAR, "SVD did not converge (non-finite values in the measurement matrix)");
  b.order.resize(k);
  descending_order(D, (size_t)k + 1, k, b.order.data());
  b.sign.resize(n_rank);
  for (int i = 0; i < n_rank; ++i) {
    const int col = b.order[i];
    int big = 0;
    for (int c = 1; c < n; ++c)
      if (std::fabs(V[(size_t)c * k + col]) > std::fabs(V[(size_t)big * k + col])) big = c;
    b.sign[i] = V[(size_t)big * k + col] < 0.0 ? -1.0 : 1.0;  // largest component positive
  }
  return MVBA_OK;
}
// component c of basis vector i
inline double basis_at(const Basis &b, const double *V, int k, int c, int i) { return b.sign[i] * V[(size_t)c * k + b.order[i]]; }
// Mg [n][4] <- basis vectors g0 .. g0 + 3, zero padded beyond n_rank: the block the projection and the depth kernels read from dMr
inline void basis_block(const Basis &b, const double *V, int k, int n, int g0, int n_rank, double *Mg) {
  for (int c = 0; c < n; ++c)
    for (int i = 0; i < 4; ++i) Mg[(size_t)c * 4 + i] = g0 + i < n_rank ? basis_at(b, V, k, c, g0 + i) : 0.0;
}

// ------------------------------------------------------------------ SVD workspace: tile sizes and dynamic LDS
// The sizes the kernels of mvsvd.hip are written for, and for every kernel that takes dynamic LDS the ONE formula of its size (the
// launch uses it) under the limit mvsvd_create raises the kernel to (set_lds_limits).  host_check.cpp holds every formula to its
// limit at the largest arguments its route admits.  `el`: bytes of an element of the workspace's dtype (4 or 8).
constexpr int GT = 16;             // Gram tile = one v_mfma_f64_16x16x4_f64 accumulator
constexpr int ROWS_PER_STEP = 32;  // rows consumed per unrolled step (8 MFMA k-groups of 4 rows)
constexpr int GRAM_ROWS = 4 * ROWS_PER_STEP;  // 128 rows per workgroup step
constexpr int WIDE_MIN = 64;     // columns above which the implicit form takes over (n <= 64: the eigenproblem sits in LDS, 6 ms)
constexpr int JACOBI_MAX = 256;  // columns up to which the Gram + Jacobi route stays available (n_rank > 16: 0.4 s of Jacobi there)
constexpr int WB = 32;           // block width of the wide path (= the small solver's order)
constexpr int JW = 32;           // max order of the small solver (k_jacobi_small: static LDS only)
constexpr int JACOBI_LDS_ORDER = 64;  // max order at which k_jacobi keeps both n x n matrices in LDS
constexpr int PC = 64;           // k_project: columns per LDS chunk
constexpr int DG_ROWS_MAX = 128;  // rows staged per pass of k_dual_gram (fewer when 3 m columns of them do not fit the LDS: dual_gram_rows)
constexpr int FZ_MAXM = 10;       // images on the fused depth path (n = 3 m <= 32)
constexpr int DEPTH_MAX_IMAGES = 768;  // k_dual_apply_wide keeps U4 and w (24 doubles per image) in LDS: 147,456 B of DEPTH_LDS_MAX
constexpr size_t LDS_DEFAULT = 64 * 1024;  // what a kernel may ask for without an attribute: the Gram forms, k_jacobi<false>
constexpr size_t JACOBI_LDS_MAX = 96 * 1024;         // k_jacobi<true>
constexpr size_t ROTATE_LDS_MAX = 64 * 1024;         // k_rotate_rows
constexpr size_t PROJECT_LDS_MAX = 160 * 1024 - 64;  // k_project
constexpr size_t DEPTH_LDS_MAX = 148 * 1024;  // the depth kernels, k_scale_rows_tiled, k_gram_xz (+ 2 KiB static in block_sum_to)
constexpr size_t TILE_MAX_BYTES = 120 * 1024;  // LDS the four tiles of a block may take (plus the small operand tables: < 160 KiB)

// The Gram forms of n <= 32 columns (k_gram_fused<T, MODE>, k_gram_xz): MODE 1 up to 16 columns, 2 (the packed tile) up to 24, 3
// up to 32; 0 = tile pair by tile pair (k_gram_pair).  A form's partial tiles: as many as its mode, else every pair of tiles.
inline int gram_mode(int n) { return n <= 16 ? 1 : (n <= 24 ? 2 : (n <= 32 ? 3 : 0)); }
inline int gram_tiles(int n) { return (n + GT - 1) / GT; }
inline int gram_pairs(int n) { return gram_mode(n) == 2 ? 2 : gram_tiles(n) * (gram_tiles(n) + 1) / 2; }
// staged rows, or the 8 KiB per partial tile of gram_store_partial
inline size_t gram_fused_lds(size_t el, int n) { return std::max<size_t>(el * GRAM_ROWS * n, (size_t)gram_pairs(n) * 8192); }
// k_gram_xz of m images: GRAM_ROWS rows of sx [3 m] | sz [m] | sp [m] | (with the rotation) B = W V1 [3 m]
inline size_t gram_xz_lds(int m, bool rot) {
  return std::max<size_t>(sizeof(double) * (size_t)GRAM_ROWS * ((rot ? 2 : 1) * 3 * m + 2 * m), (size_t)gram_pairs(3 * m) * 8192);
}
// k_jacobi: the rotations of a step; up to JACOBI_LDS_ORDER also A and V
inline size_t jacobi_lds(int n) {
  const int np = (n + 1) & ~1;
  if (n <= JW) return 0;
  return sizeof(double) * (3 * (np / 2) + 2) + 16 + (n <= JACOBI_LDS_ORDER ? sizeof(double) * 2 * (size_t)n * n : 0);
}
inline size_t rotate_rows_lds(size_t el, int n) { return (size_t)GRAM_ROWS * n * el; }
// The two route decisions of a factorisation (run() in mvsvd.hip; restated in tests/_svd_cases.py).
// A workspace of more than WIDE_MIN columns (`wide`) takes the block iteration for up to WB / 2 triplets, and beyond JACOBI_MAX
// columns for any (where it refuses more); otherwise the Gram + Jacobi route.
inline bool wide_route(bool wide, int n, int n_rank) { return wide && (n_rank <= WB / 2 || n > JACOBI_MAX); }
// The second pass rotates a tall and narrow matrix in the streaming form (k_rotate_rows: whole 16-byte vectors per row, an even
// number of columns on the two column tiles); every other shape goes through the 64 x 64 tiles of k_rotate.
inline bool rotate_streams(size_t el, long long n_rows, int n) { return n <= 32 && n % 2 == 0 && (n * el) % 16 == 0 && n_rows >= 4096; }
// k_project: 4 n doubles (unused), mu [n], four tiles of 64 rows x min(n, PC) columns at an odd stride
inline size_t project_lds(size_t el, int n) { return sizeof(double) * (5 * (size_t)n) + el * 4 * 64 * (size_t)(std::min(n, PC) | 1) + 16; }
// four wave tiles of 64 rows x cols elements at an odd stride: k_scale_rows_tiled (cols = n + groups), the tiled depth kernels (4 m)
inline size_t row_tile_lds(size_t el, int cols) { return el * 4 * 64 * (size_t)(cols | 1); }
inline bool tile_fits(size_t el, int cols) { return row_tile_lds(el, cols) <= TILE_MAX_BYTES; }
// the depth update of m images goes through row tiles (coalesced) while they and the dual method's 24 doubles per image fit
inline bool depth_tiled(size_t el, int m) { return tile_fits(el, 4 * m) && 24 * m * sizeof(double) <= 24 * 1024; }
// k_depth_primary, k_primary_xz: U [3 m][4] and the tiles; k_depth_primary_wide: U and per wave [64][10 sums | 4 components]
inline size_t depth_primary_lds(size_t el, int m) { return sizeof(double) * 12 * m + row_tile_lds(el, 4 * m) + 16; }
inline size_t depth_primary_wide_lds(int m) { return sizeof(double) * (12 * (size_t)m + 4 * 64 * 14); }
// k_dual_apply, k_dual_apply_xz: U4 [3 m][4], w [m][12] and the tiles; k_dual_apply_wide: the two tables alone
inline size_t dual_apply_lds(size_t el, int m) { return sizeof(double) * 24 * m + row_tile_lds(el, 4 * m) + 16; }
inline size_t dual_apply_wide_lds(int m) { return sizeof(double) * 24 * m; }
// k_dual_gram stages [rows][3 m | 1] normalised observations + [rows][4] right singular vectors per pass
inline int dual_gram_rows(int m) { return (int)std::max<size_t>(1, std::min<size_t>(DG_ROWS_MAX, DEPTH_LDS_MAX / (sizeof(double) * (size_t)(((3 * m) | 1) + 4)))); }
inline size_t dual_gram_lds(int m, int rows) { return sizeof(double) * ((size_t)rows * (((3 * m) | 1) + 4)); }
// k_dual_gram_mfma<M>: U [3 m][4]; per wave ROWS_PER_STEP rows of x [3 m] | z [m] | V4 [4] and the four planes [row][m | 1] + 8
// of S's shares
inline size_t dual_gram_mfma_lds(int m) {
  return sizeof(double) * (12 * (size_t)m + 4 * ((size_t)ROWS_PER_STEP * (4 * m + 4) + 4 * ((size_t)ROWS_PER_STEP * (m | 1) + 8)));
}

// The depth iteration's scratch (ddep) for m images.  Both routes start it the same way,
//   [blocks] error partials | [8] error | G12 [m][144] | V12 [m][144] | colsum [m][12] | w12 [m][12]
// and keep their own partial sums behind that, from `own` on.
struct DepthScratch {
  double *Epart = nullptr, *Eout = nullptr, *G12 = nullptr, *V12 = nullptr, *colsum = nullptr, *w12 = nullptr, *own = nullptr;
  DepthScratch() = default;
  static size_t prefix(int blocks, int m) { return (size_t)blocks + 8 + (size_t)m * (144 + 144 + 12 + 12); }
  DepthScratch(double *ddep, int blocks, int m)
      : Epart(ddep), Eout(Epart + blocks), G12(Eout + 8), V12(G12 + (size_t)m * 144), colsum(V12 + (size_t)m * 144),
        w12(colsum + (size_t)m * 12), own(w12 + (size_t)m * 12) {}
};

}  // namespace mvba
