// The SVD workspace's host arithmetic (mvba_host.h: select_basis, basis_block, DepthScratch) on hand-made inputs.  A program of
// its own, meant for the host sanitizers (`make host_check`); it makes no HIP call and needs no GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "mvba_host.h"

namespace mvba {
thread_local std::string g_err;
}
using namespace mvba;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("host_check: line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

int main() {
  {  // 1. ties: two equal eigenvalues keep no promise about their order, two components of equal magnitude take the FIRST as the largest
    const int n = 3;
    const double D[9] = {1.0, 0, 0, 0, 4.0, 0, 0, 0, 2.0};
    const double V[9] = {-0.5, 0.6, 0.0,   // rows are components, columns are vectors
                         0.5, -0.8, -1.0,  //
                         0.5, 0.8, 1.0};
    Basis b;
    CHECK(select_basis(D, V, n, n, 2, b) == MVBA_OK);
    CHECK(b.order.size() == 3 && b.order[0] == 1 && b.order[1] == 2 && b.order[2] == 0);
    CHECK(b.sign.size() == 2);
    CHECK(b.sign[0] == -1.0);  // vector 1 = (0.6, -0.8, 0.8): |-0.8| = |0.8|, the first of the two is negative
    CHECK(b.sign[1] == -1.0);  // vector 2 = (0, -1, 1)
    CHECK(basis_at(b, V, n, 1, 0) == 0.8 && basis_at(b, V, n, 2, 0) == -0.8);
    std::vector<double> Mg((size_t)n * 4, -7.0);
    basis_block(b, V, n, n, 0, 2, Mg.data());
    const double want[12] = {-0.6, -0.0, 0, 0, 0.8, 1.0, 0, 0, -0.8, -1.0, 0, 0};
    for (int i = 0; i < 12; ++i) CHECK(Mg[i] == want[i]);
    Basis t;  // the sign of the third vector (-0.5, 0.5, 0.5): the first of three equal magnitudes
    CHECK(select_basis(D, V, n, n, 3, t) == MVBA_OK && t.sign[2] == -1.0);
  }
  {  // 2. a NaN eigenvalue: refused before anything is ordered, with numpy's words
    const int n = 2;
    const double D[4] = {1.0, 0, 0, std::numeric_limits<double>::quiet_NaN()};
    const double V[4] = {1, 0, 0, 1};
    Basis b;
    g_err.clear();
    CHECK(select_basis(D, V, n, n, 1, b) == MVBA_ERR_SINGULAR);
    CHECK(g_err == "SVD did not converge (non-finite values in the measurement matrix)");
    const double Dinf[4] = {std::numeric_limits<double>::infinity(), 0, 0, 1.0};
    CHECK(select_basis(Dinf, V, n, n, 1, b) == MVBA_ERR_SINGULAR);
  }
  {  // 3. n_rank = n, more than one block of four, and a tall V (n rows, k < n vectors: the wide route's shape)
    const int n = 6;
    std::vector<double> D((size_t)n * n, 0.0), V((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
      D[(size_t)i * n + i] = i + 1.0;                      // ascending: the order is the reverse
      V[(size_t)((i + 1) % n) * n + i] = i % 2 ? -1 : 1;  // vector i = +-e_(i+1)
    }
    Basis b;
    CHECK(select_basis(D.data(), V.data(), n, n, n, b) == MVBA_OK);
    for (int i = 0; i < n; ++i) CHECK(b.order[i] == n - 1 - i && b.sign[i] == ((n - 1 - i) % 2 ? -1.0 : 1.0));
    std::vector<double> Mg((size_t)n * 4);
    for (int g0 = 0; g0 < n; g0 += 4) {
      basis_block(b, V.data(), n, n, g0, n, Mg.data());
      for (int c = 0; c < n; ++c)
        for (int i = 0; i < 4; ++i) CHECK(Mg[(size_t)c * 4 + i] == (g0 + i < n && c == (b.order[g0 + i] + 1) % n ? 1.0 : 0.0));
    }
    const int k = 2, rows = 5;
    const double Dk[4] = {3.0, 0, 0, 9.0};
    const double Vk[rows * k] = {0.1, 0.2, 0.3, -0.9, -0.7, 0.1, 0.2, 0.3, 0.6, 0.2};
    Basis w;
    CHECK(select_basis(Dk, Vk, k, rows, 2, w) == MVBA_OK);
    CHECK(w.order[0] == 1 && w.order[1] == 0 && w.sign[0] == -1.0 && w.sign[1] == -1.0);
    std::vector<double> Mw((size_t)rows * 4);
    basis_block(w, Vk, k, rows, 0, 2, Mw.data());
    CHECK(Mw[1 * 4 + 0] == 0.9 && Mw[2 * 4 + 1] == 0.7 && Mw[4 * 4 + 2] == 0.0 && Mw[4 * 4 + 3] == 0.0);
  }
  {  // the depth scratch: every part inside prefix(), in order, `own` right behind it
    const int blocks = 2048, m = 3;
    std::vector<double> buf(DepthScratch::prefix(blocks, m) + 5, 0.0);
    const DepthScratch d(buf.data(), blocks, m);
    CHECK(d.Epart == buf.data() && d.Eout == d.Epart + blocks && d.G12 == d.Eout + 8 && d.V12 == d.G12 + 144 * m);
    CHECK(d.colsum == d.V12 + 144 * m && d.w12 == d.colsum + 12 * m && d.own == d.w12 + 12 * m);
    CHECK(d.own == buf.data() + DepthScratch::prefix(blocks, m));
    for (double *p = d.Epart; p < d.own + 5; ++p) *p = 1.0;  // (every double of it is the vector's)
    CHECK(DepthScratch().own == nullptr);
  }
  if (failures) return 1;
  std::printf("host_check ok\n");
  return 0;
}
