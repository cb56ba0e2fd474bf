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
