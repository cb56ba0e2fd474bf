// The SVD workspace's host arithmetic (mvba_host.h: select_basis, basis_block, DepthScratch, the LDS formulas), the BA engine's host
// logic (mvba_engine_host.h: build_parameter_map, reduced_system_residual, expand_packed_A, expand_compact_record and the record_to_*
// fills of mvba_debug_read, the cam15 row, the lane form's packed index row and range count, the width rules of K5, the cost pass and the covariance) and the host logic of a RANSAC
// round (mvba_ransac_host.h: rs_pick, rs_accept, rs_current and rs_other, RsTile, CamChunks, the argument checks, the homography's hg_*, align_solve) and the track
// builder's host pieces (mvba_tracks_host.h: its argument checks, tracks_classify, trk_grid) and the matcher's (mvba_match_host.h: its
// argument checks, the chunk rule, the ratio test, the plan of a call and the block lists of a chunk) and lap_rest on hand-made inputs.  A program of its own,
// meant for the host sanitizers (`make host_check`); it makes no HIP call and needs no GPU.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <limits>
#include <string>
#include <vector>

#include "mvba_host.h"
#include "mvba_engine_host.h"
#include "mvba_ransac_host.h"
#include "mvba_tracks_host.h"
#include "mvba_match_host.h"

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
  {  // the SVD workspace's LDS formulas at the largest arguments their routes admit, each within the limit its kernel is raised to
    for (size_t el : {(size_t)4, (size_t)8}) {
      for (int n = 1; n <= 32; ++n) CHECK(gram_mode(n) >= 1 && gram_pairs(n) == gram_mode(n) && gram_fused_lds(el, n) <= LDS_DEFAULT);
      CHECK(gram_fused_lds(el, 32) == std::max<size_t>(el * 128 * 32, 3 * 8192));
      CHECK(rotate_rows_lds(el, 32) <= ROTATE_LDS_MAX);  // the streaming form of mvsvd_run: n <= 32; the wide path: WB fp64 columns
      CHECK(project_lds(el, JACOBI_MAX) <= PROJECT_LDS_MAX && project_lds(el, PC) == project_lds(el, JACOBI_MAX) - 5 * sizeof(double) * (JACOBI_MAX - PC));
      int cols = 1;  // the widest rows that go through tiles
      while (tile_fits(el, cols + 1)) ++cols;
      CHECK(cols == (el == 8 ? 59 : 119) && !tile_fits(el, cols + 1) && row_tile_lds(el, cols) <= TILE_MAX_BYTES && row_tile_lds(el, cols) <= DEPTH_LDS_MAX);
      int mt = 1;  // the most images whose depth update is tiled
      while (depth_tiled(el, mt + 1)) ++mt;
      CHECK(mt == cols / 4 && !depth_tiled(el, mt + 1));
      CHECK(depth_primary_lds(el, mt) <= DEPTH_LDS_MAX && dual_apply_lds(el, mt) <= DEPTH_LDS_MAX);
      CHECK(dual_apply_lds(el, mt) == 24 * 8 * (size_t)mt + row_tile_lds(el, 4 * mt) + 16);
    }
    CHECK(depth_tiled(8, 14) && !depth_tiled(8, 15) && depth_tiled(4, 29) && !depth_tiled(4, 30));
    CHECK(gram_mode(33) == 0 && gram_pairs(33) == 6 && gram_pairs(JACOBI_MAX) == 136 && gram_tiles(17) == 2);
    CHECK(rotate_rows_lds(8, WB) <= ROTATE_LDS_MAX);
    CHECK(jacobi_lds(JW) == 0 && jacobi_lds(JW + 1) > 0);
    CHECK(jacobi_lds(JACOBI_LDS_ORDER) == 8 * (3 * 32 + 2) + 16 + 16 * 64 * 64 && jacobi_lds(JACOBI_LDS_ORDER) <= JACOBI_LDS_MAX);  // k_jacobi<true>: above the default
    CHECK(jacobi_lds(JACOBI_LDS_ORDER) > LDS_DEFAULT && jacobi_lds(JACOBI_LDS_ORDER + 1) < jacobi_lds(JACOBI_LDS_ORDER) && jacobi_lds(JACOBI_MAX) <= LDS_DEFAULT);
    for (int m = 2; m <= FZ_MAXM; m += 2) {  // the fused depth iteration: fp64, its tiles are not asked whether they fit
      CHECK(3 * m <= 32 && tile_fits(8, 4 * m));
      for (bool rot : {false, true}) CHECK(gram_xz_lds(m, rot) <= DEPTH_LDS_MAX);
      CHECK(depth_primary_lds(8, m) <= DEPTH_LDS_MAX && dual_apply_lds(8, m) <= DEPTH_LDS_MAX && dual_gram_mfma_lds(m) <= DEPTH_LDS_MAX);
    }
    CHECK(gram_xz_lds(FZ_MAXM, true) == 8 * 128 * 80 && gram_xz_lds(2, false) == 8 * 128 * 10 && gram_xz_lds(1, false) == 8192);
    CHECK(dual_gram_mfma_lds(FZ_MAXM) == 8 * (120 + 4 * (32 * 44 + 4 * (32 * 11 + 8))));
    CHECK(depth_primary_wide_lds(DEPTH_MAX_IMAGES) <= DEPTH_LDS_MAX && dual_apply_wide_lds(DEPTH_MAX_IMAGES) <= DEPTH_LDS_MAX);
    CHECK(dual_apply_wide_lds(DEPTH_MAX_IMAGES) == 147456);
    for (int m = 1; m <= DEPTH_MAX_IMAGES; ++m) {  // k_dual_gram: at least one row, and what it stages fits
      const int rows = dual_gram_rows(m);
      CHECK(rows >= 1 && rows <= DG_ROWS_MAX && dual_gram_lds(m, rows) <= DEPTH_LDS_MAX);
      CHECK(rows == DG_ROWS_MAX || dual_gram_lds(m, rows + 1) > DEPTH_LDS_MAX);  // (as many as fit)
    }
    CHECK(dual_gram_rows(47) == 128 && dual_gram_rows(48) < 128 && dual_gram_rows(256) == 24);
  }
  {  // the two route decisions of run() at their edges
    // the block iteration: a wide workspace (more than WIDE_MIN columns) asked for up to WB / 2 triplets, or beyond JACOBI_MAX columns for any
    CHECK(!wide_route(false, WIDE_MIN, 1) && !wide_route(false, WIDE_MIN, 16) && !wide_route(false, WIDE_MIN, 17));  // (create_workspace: wide = n > WIDE_MIN)
    CHECK(wide_route(true, WIDE_MIN + 1, 1) && wide_route(true, WIDE_MIN + 1, WB / 2) && !wide_route(true, WIDE_MIN + 1, WB / 2 + 1));
    CHECK(wide_route(true, JACOBI_MAX, 16) && !wide_route(true, JACOBI_MAX, 17) && !wide_route(true, JACOBI_MAX, JACOBI_MAX));
    CHECK(wide_route(true, JACOBI_MAX + 1, 16) && wide_route(true, JACOBI_MAX + 1, 17));  // (run_wide refuses the 17)
    CHECK(WB / 2 == 16 && WIDE_MIN == 64 && JACOBI_MAX == 256);
    // the streaming rotation: even n <= 32 whose rows are whole 16-byte vectors, from 4096 rows on
    for (int n = 1; n <= 40; ++n) {
      CHECK(rotate_streams(8, 4096, n) == (n % 2 == 0 && n <= 32));
      CHECK(rotate_streams(4, 4096, n) == (n % 4 == 0 && n <= 32));
      CHECK(!rotate_streams(8, 4095, n) && !rotate_streams(4, 4095, n));
      if (rotate_streams(8, 4096, n)) CHECK(rotate_rows_lds(8, n) <= ROTATE_LDS_MAX && (GRAM_ROWS * n) % 2 == 0);
    }
    CHECK(rotate_streams(8, 4096, 2) && rotate_streams(8, 4096, 32) && !rotate_streams(8, 4096, 34) && !rotate_streams(8, 4096, 31));
    CHECK(rotate_streams(8, 1LL << 40, 32) && !rotate_streams(8, 1, 32));
  }
  {  // the pick of a count row: ties, all degenerate, below the minimum, a small item, H = 1
    const int ON = RS_OK | RS_ACTIVE | RS_CUR;
    const int tie[5] = {3, 9, -1, 9, 2};
    RsPick k = rs_pick(tie, 5, 100, 8);
    CHECK(k.best == 1 && k.status == 0 && k.state == ON);  // the first of the two nines
    const int none[3] = {-1, -1, -1};
    k = rs_pick(none, 3, 100, 6);
    CHECK(k.best == -1 && k.status == 2 && k.state == 0);
    const int low[4] = {-1, 5, 4, 5};
    k = rs_pick(low, 4, 100, 6);
    CHECK(k.best == 1 && k.status == 4 && k.state == 0);
    CHECK(rs_pick(low, 4, 100, 4).status == 0);  // (the pose's minimum)
    k = rs_pick(none, 3, 5, 6);  // an item below the minimum scores nothing: every count is -1
    CHECK(k.best == -1 && k.status == 1 && k.state == 0);
    CHECK(rs_pick(none, 3, 3, 4).status == 1 && rs_pick(none, 3, 7, 8).status == 1);
    const int one[1] = {12};
    k = rs_pick(one, 1, 12, 8);
    CHECK(k.best == 0 && k.status == 0 && k.state == ON);
    const int one_bad[1] = {-1};
    CHECK(rs_pick(one_bad, 1, 12, 8).best == -1 && rs_pick(one_bad, 1, 12, 8).status == 2);
  }
  {  // the accept rule: two-view and pose have no first-refit minimum (0), the DLT's is 6
    for (long long first_min : {0LL, 0LL, 6LL})
      for (int r : {0, 1, 5}) {
        if (first_min && r == 0) continue;  // (the DLT's first refit: below)
        int st = RS_OK | RS_ACTIVE, n_active = 3;
        CHECK(rs_accept(40, 40, r, first_min, st, n_active));  // an equal count is kept: the other buffer becomes current
        CHECK(st == (RS_OK | RS_ACTIVE | RS_CUR) && n_active == 3);
        CHECK(rs_accept(41, 40, r, first_min, st, n_active) && st == (RS_OK | RS_ACTIVE) && n_active == 3);
        CHECK(!rs_accept(39, 40, r, first_min, st, n_active));  // one smaller: stops, on the buffer it had
        CHECK(st == RS_OK && n_active == 2);
      }
    int st = RS_OK | RS_ACTIVE | RS_CUR, n_active = 1;
    CHECK(rs_accept(6, 40, 0, 6, st, n_active) && st == (RS_OK | RS_ACTIVE) && n_active == 1);  // the DLT's first refit: 6 against 40
    CHECK(!rs_accept(5, 40, 0, 6, st, n_active) && st == RS_OK && n_active == 0);
    st = RS_OK | RS_ACTIVE; n_active = 1;
    CHECK(!rs_accept(6, 40, 1, 6, st, n_active) && n_active == 0);  // its second is held to the kept count
    st = RS_OK | RS_ACTIVE | RS_CUR; n_active = 2;
    rs_stop(st, n_active);
    CHECK(st == (RS_OK | RS_CUR) && n_active == 1);
  }
  {  // the two mask buffers under the state: the first mask goes to buffer 0, a toggle makes it current, a refit writes the other
    unsigned char b0[1], b1[1];
    const unsigned char *c0 = b0, *c1 = b1;
    const int nine[1] = {9};
    int st = rs_pick(nine, 1, 9, 8).state;
    CHECK(rs_other(st, b0, b1) == b0 && rs_current(st, c0, c1) == c1);
    st ^= RS_CUR;
    CHECK(rs_current(st, b0, b1) == b0 && rs_other(st, b0, b1) == b1 && rs_current(st, c0, c1) == c0);
    int n_active = 1;
    CHECK(rs_accept(9, 9, 0, 0, st, n_active) && rs_current(st, b0, b1) == b1 && rs_other(st, b0, b1) == b0);  // kept: the other became current
    CHECK(!rs_accept(8, 9, 1, 0, st, n_active) && rs_current(st, b0, b1) == b1);                                 // stopped: it stays
  }
  {  // RsTile: a tile of four items with the statuses 1, 2, 4 and 0, three hypotheses each
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int ON = RS_OK | RS_ACTIVE | RS_CUR;
    const int H = 3, hc[12] = {-1, -1, -1, -1, -1, -1, -1, 5, 4, 7, 9, 9}, n_item[4] = {5, 100, 100, 100};
    int32_t status[5], best[5], hyp_count[15];
    int64_t n_it[5], n_inl[5];
    double quality[10];
    for (int g = 0; g < 5; ++g) { status[g] = best[g] = 77; n_it[g] = n_inl[g] = 77; quality[2 * g] = quality[2 * g + 1] = 77.0; }
    for (int &c : hyp_count) c = 77;
    RsTile::defaults(5, H, status, best, hyp_count, n_it, n_inl, quality);
    for (int g = 0; g < 5; ++g)
      CHECK(status[g] == 1 && best[g] == -1 && n_it[g] == 0 && n_inl[g] == 0 && std::isnan(quality[2 * g]) && std::isnan(quality[2 * g + 1]));
    for (int c : hyp_count) CHECK(c == -1);
    RsTile t(4);
    int state[4] = {77, 77, 77, 77};
    t.pick(4, state, hc, H, n_item, 6);
    const int want_st[4] = {1, 2, 4, 0}, want_best[4] = {-1, -1, 1, 1}, want_state[4] = {0, 0, 0, ON};
    for (int p = 0; p < 4; ++p) CHECK(t.st[p] == want_st[p] && t.best[p] == want_best[p] && state[p] == want_state[p]);
    const double S2[8] = {nan, nan, nan, nan, nan, nan, 9.0, 36.0};  // (the mask pass sums nothing for an item that is out)
    int calls = 0;
    CHECK(t.first(S2, [&](int p) { ++calls; CHECK(p == 3); return 0; }) == 1 && calls == 1 && t.n_active == 1);
    CHECK(state[0] == 0 && state[1] == 0 && state[2] == 0 && state[3] == (RS_OK | RS_ACTIVE) && t.nin[3] == 9 && t.ssq[3] == 36.0);
    calls = 0;
    t.write(1, status, best, hyp_count, n_inl, quality, [&](int p) { ++calls; CHECK(p == 3); return 0.25; });  // the tile starts at item 1
    CHECK(calls == 1 && status[0] == 1 && best[0] == -1 && hyp_count[0] == -1);  // (item 0 is not the tile's)
    for (int p = 0; p < 4; ++p) {
      CHECK(status[1 + p] == want_st[p] && best[1 + p] == want_best[p]);
      for (int h = 0; h < H; ++h) CHECK(hyp_count[(1 + p) * H + h] == hc[p * H + h]);
      if (p < 3) CHECK(n_inl[1 + p] == 0 && std::isnan(quality[2 * (1 + p)]) && std::isnan(quality[2 * (1 + p) + 1]));  // the defaults stay
    }
    CHECK(n_inl[4] == 9 && quality[8] == 2.0 && quality[9] == 0.25);

    // a finish that fails for one of two items of status 0: it is out with finish's status, the other goes on
    const int hc2[6] = {8, 3, 1, 2, 9, 9}, n2[2] = {50, 50};
    int state2[2];
    RsTile u(3);  // (a tile may be shorter than the one the vectors were made for)
    u.pick(2, state2, hc2, H, n2, 6);
    CHECK(u.st[0] == 0 && u.st[1] == 0 && u.best[0] == 0 && u.best[1] == 1 && state2[0] == ON && state2[1] == ON);
    const double S2b[4] = {8.0, 2.0, 9.0, 4.5};
    CHECK(u.first(S2b, [](int p) { return p == 0 ? 2 : 0; }) == 1);
    CHECK(u.st[0] == 2 && state2[0] == 0 && u.st[1] == 0 && state2[1] == (RS_OK | RS_ACTIVE) && u.nin[1] == 9);
    int kept = 0;
    u.accept(0, std::vector<double>{nan, nan, 9.0, 4.0}.data(), 0, [&](int p) { ++kept; CHECK(p == 1); });  // item 0 is not asked again
    CHECK(kept == 1 && state2[0] == 0 && u.n_active == 1);

    // accept: an equal count is kept and the buffer toggles; one fewer stops on the buffer it had
    u.pick(2, state2, hc2, H, n2, 6);
    CHECK(u.first(S2b, [](int) { return 0; }) == 2);
    kept = 0;
    u.accept(0, std::vector<double>{8.0, 1.0, 8.0, 1.0}.data(), 0, [&](int p) { ++kept; CHECK(p == 0); });
    CHECK(kept == 1 && u.n_active == 1 && state2[0] == ON && u.nin[0] == 8 && u.ssq[0] == 1.0);
    CHECK(state2[1] == RS_OK && u.nin[1] == 9 && u.ssq[1] == 4.5);
    u.accept(1, std::vector<double>{9.0, 3.0, 50.0, 0.0}.data(), 0, [&](int p) { ++kept; CHECK(p == 0); });  // (a stopped item's sums are not looked at)
    CHECK(kept == 2 && state2[0] == (RS_OK | RS_ACTIVE) && u.nin[0] == 9 && u.ssq[0] == 3.0 && state2[1] == RS_OK && u.nin[1] == 9);

    // a first_min: refit 0 is held to it, not to the kept count; refit 1 to the count refit 0 left
    u.pick(2, state2, hc2, H, n2, 6);
    u.first(std::vector<double>{40.0, 1.0, 40.0, 1.0}.data(), [](int) { return 0; });
    kept = 0;
    u.accept(0, std::vector<double>{6.0, 0.5, 5.0, 0.5}.data(), 6, [&](int p) { ++kept; CHECK(p == 0); });
    CHECK(kept == 1 && u.nin[0] == 6 && state2[0] == ON && u.nin[1] == 40 && state2[1] == RS_OK && u.n_active == 1);
    u.accept(1, std::vector<double>{6.0, 0.25, nan, nan}.data(), 6, [&](int) { ++kept; });
    CHECK(kept == 2 && u.nin[0] == 6 && u.ssq[0] == 0.25 && state2[0] == (RS_OK | RS_ACTIVE) && u.n_active == 1);
    u.accept(2, std::vector<double>{5.0, 0.125, nan, nan}.data(), 6, [&](int) { ++kept; });
    CHECK(kept == 2 && u.nin[0] == 6 && u.ssq[0] == 0.25 && state2[0] == RS_OK && u.n_active == 0);

    // n_refit = 0: what first took is what write gives, and the first mask -- buffer 0 -- is the current one; every optional
    // output null: q1 is still called; H = 1
    const int one[2] = {12, -1}, n1[2] = {12, 12};
    RsTile v(2);
    v.pick(2, state2, one, 1, n1, 8);
    CHECK(v.st[0] == 0 && v.best[0] == 0 && v.st[1] == 2 && v.best[1] == -1);
    CHECK(v.first(std::vector<double>{12.0, 48.0, nan, nan}.data(), [](int) { return 0; }) == 1);
    unsigned char b0[1], b1[1];
    CHECK(rs_current(state2[0], b0, b1) == b0 && (state2[0] & RS_OK) && state2[1] == 0);
    RsTile::defaults(2, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    calls = 0;
    v.write(0, nullptr, nullptr, nullptr, nullptr, nullptr, [&](int p) { ++calls; CHECK(p == 0); return 0.0; });
    CHECK(calls == 1);
    int32_t st1[2] = {77, 77}, hc1[2] = {77, 77};
    double q[4] = {77, 77, 77, 77};
    v.write(0, st1, nullptr, hc1, nullptr, q, [](int) { return 0.5; });
    CHECK(st1[0] == 0 && st1[1] == 2 && hc1[0] == 12 && hc1[1] == -1 && q[0] == 2.0 && q[1] == 0.5 && q[2] == 77 && q[3] == 77);
  }
  {  // the chunk list: cameras with 0, 1, 256 and 257 observations, one listed twice; cameras = NULL
    const long long cam_ptr[5] = {0, 0, 1, 257, 514};
    const int32_t cams[5] = {3, 0, 2, 3, 1};
    int64_t nu[5] = {-1, -1, -1, -1, -1};
    CamChunks w;
    CHECK(w.build(cam_ptr, cams, 5, 256, nu) == MVBA_OK);
    const int want_n[5] = {257, 0, 256, 257, 1}, want_ch[6] = {0, 2, 2, 3, 5, 6};
    const long long want_mask[5] = {0, 257, 257, 513, 770};
    for (int c = 0; c < 5; ++c)
      CHECK(w.cams[c] == cams[c] && w.lc_n[c] == want_n[c] && nu[c] == want_n[c] && w.lc_start[c] == cam_ptr[cams[c]] && w.lc_mask[c] == want_mask[c]);
    for (int c = 0; c <= 5; ++c) CHECK(w.lc_ch[c] == want_ch[c]);
    CHECK(w.n_ch == 6 && w.n_mask == 771 && w.ch_cam.size() == 6);
    const int want_cam[6] = {0, 0, 2, 3, 3, 4}, want_cnt[6] = {256, 1, 256, 256, 1, 1};
    const long long want_start[6] = {257, 513, 1, 257, 513, 0}, want_cmask[6] = {0, 256, 257, 513, 769, 770};
    for (int i = 0; i < 6; ++i)
      CHECK(w.ch_cam[i] == want_cam[i] && w.ch_cnt[i] == want_cnt[i] && w.ch_start[i] == want_start[i] && w.ch_mask[i] == want_cmask[i]);
    CHECK(w.lc_mask[0] != w.lc_mask[3]);  // the camera listed twice has two mask ranges
    CamChunks all;  // cameras = NULL: list position = camera, no n_usable
    CHECK(all.build(cam_ptr, nullptr, 4, 256, nullptr) == MVBA_OK);
    CHECK(all.n_ch == 4 && all.n_mask == 514 && all.lc_ch[1] == 0 && all.lc_ch[2] == 1 && all.lc_ch[3] == 2 && all.lc_ch[4] == 4);
    for (int c = 0; c < 4; ++c) CHECK(all.cams[c] == c && all.lc_start[c] == cam_ptr[c] && all.lc_mask[c] == cam_ptr[c]);
    CHECK(all.ch_cnt[3] == 1 && all.ch_start[3] == 513);
    CamChunks small;  // another chunk size
    CHECK(small.build(cam_ptr, nullptr, 4, 100, nullptr) == MVBA_OK && small.n_ch == 7 && small.ch_cnt[3] == 56 && small.ch_cnt[6] == 57);
    CamChunks none;
    CHECK(none.build(cam_ptr, cams, 0, 256, nullptr) == MVBA_OK && none.n_ch == 0 && none.n_mask == 0 && none.lc_ch.size() == 1);
    const long long big_ptr[3] = {0, 5, 5 + (1LL << 31)};  // a run of 2^31: refused before anything of its size is made
    CamChunks big;
    g_err.clear();
    CHECK(big.build(big_ptr, nullptr, 2, 256, nullptr) == MVBA_ERR_BADARG);
    CHECK(g_err == "camera 1 has 2147483648 usable observations: must be < 2^31");
    CHECK(big.n_ch == 0 && big.ch_cam.size() == 1);
  }
  {  // the homography's host arithmetic: adjugate, the returned form, the signs of the two mask matrices
    const double M[9] = {2, 0, 1, 1, 3, 0, 0, 1, 4}, I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double A[9], P[9];
    hg_adjugate(M, A);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        P[3 * i + j] = 0.0;
        for (int e = 0; e < 3; ++e) P[3 * i + j] += M[3 * i + e] * A[3 * e + j];
        CHECK(P[3 * i + j] == 25.0 * I9[3 * i + j]);  // det M = 25
      }
    double U[9] = {0, 3, 0, 0, 0, 0, 0, -4, 0};  // the largest entry is negative: the sign turns, |U| = 1
    CHECK(hg_unit(U) && std::fabs(U[1] + 0.6) < 1e-15 && std::fabs(U[7] - 0.8) < 1e-15);
    double T[9] = {2, 0, 0, 0, -2, 0, 0, 0, 1};  // equal magnitudes: the first decides
    CHECK(hg_unit(T) && T[0] > 0.0 && T[4] < 0.0);
    double Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, N[9] = {1, 0, 0, 0, std::numeric_limits<double>::quiet_NaN(), 0, 0, 0, 1};
    CHECK(!hg_unit(Z) && !hg_unit(N) && Z[0] == 0.0 && N[0] == 1.0);
    // a translation by (-500, 0) in pixels, returned with its largest entry positive: w = -1 everywhere, so part 0 turns back
    const double Hp[9] = {-1, 0, 500, 0, -1, 0, 0, 0, -1}, nm[8] = {320, 240, 0.01, -180, 240, 0.01, 50, 0};
    double m0[9], m1[9];
    hg_mask_parts(Hp, nm, m0, m1);
    CHECK(m0[8] == 1.0 && m0[2] == -500.0 && m0[0] == 1.0);
    CHECK(m1[8] == 1.0 && m1[2] == 500.0 && m1[0] == 1.0);  // adj(Hp) = [[1, 0, 500], [0, 1, 0], [0, 0, 1]]: w = 1 > 0 already
    const double Hq[9] = {1, 0, 0, 0, 1, 0, 0.01, 0, -1};  // w changes sign across the image: the centroid decides
    hg_mask_parts(Hq, nm, m0, m1);
    CHECK(m0[6] * nm[0] + m0[7] * nm[1] + m0[8] > 0.0 && m1[6] * nm[3] + m1[7] * nm[4] + m1[8] > 0.0);
  }
  {  // the argument checks, with their texts
    CHECK(rs_check_search(0.01, 1) == MVBA_OK && rs_check_search(0.01, RS_MAX_HYP) == MVBA_OK && rs_check_refit(0) == MVBA_OK && rs_check_refit(RS_MAX_REFIT) == MVBA_OK);
    CHECK(rs_check_search(0.0, 8) == MVBA_ERR_BADARG && g_err == "threshold = 0.000000 must be finite and > 0");
    CHECK(rs_check_search(std::numeric_limits<double>::quiet_NaN(), 8) == MVBA_ERR_BADARG);
    CHECK(rs_check_search(std::numeric_limits<double>::infinity(), 8) == MVBA_ERR_BADARG);
    CHECK(rs_check_search(0.01, 0) == MVBA_ERR_BADARG && g_err == "n_hypotheses = 0 must be in 1 .. 65536");
    CHECK(rs_check_search(0.01, 4097, 4096) == MVBA_ERR_BADARG && g_err == "n_hypotheses = 4097 must be in 1 .. 4096");
    CHECK(rs_check_refit(17) == MVBA_ERR_BADARG && g_err == "n_refit = 17 must be in 0 .. 16");
    CHECK(rs_check_refit(-1) == MVBA_ERR_BADARG);
    const int32_t cams[3] = {0, 7, 8};
    CHECK(check_camera_list(cams, 2, 8) == MVBA_OK && check_camera_list(nullptr, 8, 8) == MVBA_OK && check_camera_list(cams, 0, 8) == MVBA_OK);
    CHECK(check_camera_list(cams, 3, 8) == MVBA_ERR_BADARG && g_err.rfind("cameras[2] = 8: ", 0) == 0 && g_err.find("n_images = 8") != std::string::npos);
    CHECK(check_camera_list(nullptr, 3, 8) == MVBA_ERR_BADARG && g_err == "cameras = NULL lists every camera: n_cameras = 3 must be n_images = 8");
    double tm[4] = {-1, -1, -1, -1};
    RsLaps laps;
    laps.upload = 1.0; laps.score += 2.0; laps.refit += 3.0; laps.other += 4.0;
    laps.write(tm);
    laps.write(nullptr);
    CHECK(tm[0] == 1.0 && tm[1] == 2.0 && tm[2] == 3.0 && tm[3] == 4.0);
  }
  {  // align_solve: identity, a known similarity, collinear points, three points, rigid
    // the moments of pts under y = s Q x + tau (Q: a quarter turn about z), as the two device passes sum them
    auto moments = [](const double (*x)[3], int n, double s, bool turn, const double *tau, double (&mx)[3], double (&my)[3], double (&mom)[11]) {
      std::vector<double> y((size_t)3 * n);
      for (int i = 0; i < n; ++i) {
        const double q[3] = {turn ? -x[i][1] : x[i][0], turn ? x[i][0] : x[i][1], x[i][2]};
        for (int e = 0; e < 3; ++e) y[3 * i + e] = s * q[e] + tau[e];
      }
      for (int e = 0; e < 3; ++e) mx[e] = my[e] = 0.0;
      for (int i = 0; i < n; ++i)
        for (int e = 0; e < 3; ++e) { mx[e] += x[i][e] / n; my[e] += y[3 * i + e] / n; }
      for (double &m : mom) m = 0.0;
      for (int i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
          const double xa = x[i][a] - mx[a], ya = y[3 * i + a] - my[a];
          mom[0] += xa * xa;
          mom[1] += ya * ya;
          for (int b = 0; b < 3; ++b) mom[2 + 3 * a + b] += ya * (x[i][b] - mx[b]);
        }
    };
    const double cube[5][3] = {{0, 0, 0}, {1, 0, 0}, {0, 2, 0}, {0, 0, 4}, {1, 1, 1}}, zero[3] = {0, 0, 0}, tau[3] = {10, -3, 4};
    double mx[3], my[3], mom[11], sim[13], gap;
    moments(cube, 5, 1.0, false, zero, mx, my, mom);
    CHECK(align_solve(mx, my, mom, true, sim, gap) == 0 && gap > 0.1);
    const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    CHECK(std::fabs(sim[0] - 1.0) < 1e-15);
    for (int e = 0; e < 9; ++e) CHECK(std::fabs(sim[1 + e] - I9[e]) < 1e-15);
    for (int e = 0; e < 3; ++e) CHECK(std::fabs(sim[10 + e]) < 1e-14);
    moments(cube, 5, 2.5, true, tau, mx, my, mom);  // s = 2.5, a quarter turn, tau
    CHECK(align_solve(mx, my, mom, true, sim, gap) == 0);
    const double Qz[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    CHECK(std::fabs(sim[0] - 2.5) < 1e-14);
    for (int e = 0; e < 9; ++e) CHECK(std::fabs(sim[1 + e] - Qz[e]) < 1e-15);
    for (int e = 0; e < 3; ++e) CHECK(std::fabs(sim[10 + e] - tau[e]) < 1e-13);
    CHECK(align_solve(mx, my, mom, false, sim, gap) == 0 && sim[0] == 1.0);  // rigid: s is exactly 1, the rotation the same
    for (int e = 0; e < 9; ++e) CHECK(std::fabs(sim[1 + e] - Qz[e]) < 1e-15);
    for (int e = 0; e < 3; ++e) CHECK(std::fabs(sim[10 + e] - (my[e] - (Qz[3 * e] * mx[0] + Qz[3 * e + 1] * mx[1] + Qz[3 * e + 2] * mx[2]))) < 1e-14);
    moments(cube, 3, 2.5, true, tau, mx, my, mom);  // three points: the minimal sample
    CHECK(align_solve(mx, my, mom, true, sim, gap) == 0 && std::fabs(sim[0] - 2.5) < 1e-14 && std::fabs(sim[2] + 1.0) < 1e-15);
    const double line[4][3] = {{0, 0.25, 1}, {0.5, 0.5, 0.875}, {1, 0.75, 0.75}, {-2, -0.75, 1.5}};  // on a line: the rotation about it is free
    moments(line, 4, 2.5, true, tau, mx, my, mom);
    CHECK(align_solve(mx, my, mom, true, sim, gap) == 2 && gap <= INIT_REL_PIVOT && std::isnan(sim[0]) && std::isnan(sim[12]));
    const double same[3][3] = {{1, 2, 3}, {1, 2, 3}, {1, 2, 3}};  // coincident: no spread at all
    moments(same, 3, 2.5, true, tau, mx, my, mom);
    CHECK(align_solve(mx, my, mom, true, sim, gap) == 2 && std::isnan(gap));
    moments(cube, 5, 2.5, true, tau, mx, my, mom);
    mom[4] = std::numeric_limits<double>::quiet_NaN();  // a moment that is not finite
    CHECK(align_solve(mx, my, mom, true, sim, gap) == 2 && std::isnan(sim[0]));
  }
  {  // mvba_build_tracks: the class of a component from (size, min_length, n_images), the first rule that holds
    CHECK(tracks_classify(1, 2, 8) == TRK_SINGLETON && tracks_classify(1, 2, 1) == TRK_SINGLETON && tracks_classify(0, 2, 8) == TRK_SINGLETON);
    CHECK(tracks_classify(2, 2, 8) == TRK_CANDIDATE && tracks_classify(8, 2, 8) == TRK_CANDIDATE && tracks_classify(9, 2, 8) == TRK_OVERSIZE);
    CHECK(tracks_classify(2, 3, 8) == TRK_SHORT && tracks_classify(3, 3, 8) == TRK_CANDIDATE);
    CHECK(tracks_classify(2, 2, 1) == TRK_OVERSIZE);                                       // one image: every match is a conflict
    CHECK(tracks_classify(5, 10, 3) == TRK_SHORT && tracks_classify(10, 10, 3) == TRK_OVERSIZE);  // short before oversize
    CHECK(tracks_classify(2147483647, 2, 2147483647) == TRK_CANDIDATE && tracks_classify(2147483647, 2, 2147483646) == TRK_OVERSIZE);
    for (int size = 1; size <= 12; ++size)
      for (int ml = 2; ml <= 12; ++ml)
        for (int m = 1; m <= 12; ++m) {
          const int c = tracks_classify(size, ml, m);
          CHECK((c == TRK_CANDIDATE) == (size >= 2 && size >= ml && size <= m));
        }
  }
  {  // its checks, with their texts: kp_ptr, then the arguments in the order the entry point looks at them
    const int64_t kp[4] = {0, 2, 2, 5}, down[4] = {0, 3, 2, 5}, off[3] = {1, 2, 3}, big[2] = {0, 1LL << 31}, most[2] = {0, (1LL << 31) - 1};
    CHECK(tracks_check_kp_ptr(3, kp) == MVBA_OK && tracks_check_kp_ptr(1, most) == MVBA_OK);
    CHECK(tracks_check_kp_ptr(0, kp) == MVBA_ERR_BADARG && g_err == "n_images = 0 must be at least 1");
    CHECK(tracks_check_kp_ptr(2, off) == MVBA_ERR_BADARG && g_err == "kp_ptr[0] = 1 must be 0");
    CHECK(tracks_check_kp_ptr(3, down) == MVBA_ERR_BADARG && g_err == "kp_ptr is not ascending: kp_ptr[2] = 2 after 3");
    CHECK(tracks_check_kp_ptr(1, big) == MVBA_ERR_BADARG && g_err == "n_nodes = kp_ptr[n_images] = 2147483648 must be < 2^31");
    const int32_t edges[6] = {0, 4, 3, 3, 4, 1}, high[4] = {0, 4, 5, 1}, low[4] = {0, 4, 2, -1};
    const double kxy[10] = {0};
    int64_t pt[3], counts[TRK_N_COUNTS];
    int32_t cam[5], node[5], track[5];
    double xy[10];
    auto run = [&](const int64_t *kp_, const double *kxy_, const int32_t *e, int64_t ne, int32_t ml, int64_t *pt_, int32_t *cam_, int32_t *node_,
                   double *xy_, int32_t *track_, int64_t *cnt_) { return tracks_check_args(3, kp_, kxy_, e, ne, ml, pt_, cam_, node_, xy_, track_, cnt_); };
    CHECK(run(kp, kxy, edges, 3, 2, pt, cam, node, xy, track, counts) == MVBA_OK);
    CHECK(run(kp, nullptr, edges, 3, 2, pt, cam, node, nullptr, track, counts) == MVBA_OK);  // no coordinates wanted
    CHECK(run(kp, kxy, nullptr, 0, 2, pt, cam, node, xy, track, counts) == MVBA_OK);         // no edges: the pointer is not looked at
    CHECK(run(nullptr, kxy, edges, 3, 2, pt, cam, node, xy, track, counts) == MVBA_ERR_BADARG && g_err == "null argument: kp_ptr (argument 2)");
    CHECK(run(kp, kxy, edges, 3, 2, nullptr, cam, node, xy, track, counts) == MVBA_ERR_BADARG && g_err == "null argument: pt_ptr (argument 8)");
    CHECK(run(kp, kxy, edges, 3, 2, pt, nullptr, node, xy, track, counts) == MVBA_ERR_BADARG && g_err == "null argument: cam_idx (argument 9)");
    CHECK(run(kp, kxy, edges, 3, 2, pt, cam, nullptr, xy, track, counts) == MVBA_ERR_BADARG && g_err == "null argument: obs_node (argument 10)");
    CHECK(run(kp, kxy, edges, 3, 2, pt, cam, node, xy, nullptr, counts) == MVBA_ERR_BADARG && g_err == "null argument: node_track (argument 12)");
    CHECK(run(kp, kxy, edges, 3, 2, pt, cam, node, xy, track, nullptr) == MVBA_ERR_BADARG && g_err == "null argument: counts (argument 13)");
    CHECK(run(kp, nullptr, edges, 3, 2, pt, cam, node, xy, track, counts) == MVBA_ERR_BADARG && g_err == "null argument: kp_xy (argument 3) with an xy to fill");
    CHECK(run(kp, kxy, edges, -1, 2, pt, cam, node, xy, track, counts) == MVBA_ERR_BADARG && g_err == "n_edges = -1: negative size");
    CHECK(run(kp, kxy, nullptr, 3, 2, pt, cam, node, xy, track, counts) == MVBA_ERR_BADARG && g_err == "null argument: edges (argument 4) with n_edges = 3");
    CHECK(run(kp, kxy, edges, 3, 1, pt, cam, node, xy, track, counts) == MVBA_ERR_BADARG && g_err == "min_length = 1 must be at least 2");
    CHECK(run(down, kxy, edges, 3, 2, pt, cam, node, xy, track, counts) == MVBA_ERR_BADARG && g_err.rfind("kp_ptr is not ascending", 0) == 0);
    CHECK(run(kp, kxy, high, 2, 2, pt, cam, node, xy, track, counts) == MVBA_ERR_BADARG && g_err == "edges[1][0] = 5: node id out of range, n_nodes = 5");
    CHECK(run(kp, kxy, low, 2, 2, pt, cam, node, xy, track, counts) == MVBA_ERR_BADARG && g_err == "edges[1][1] = -1: node id out of range, n_nodes = 5");
    CHECK(run(kp, kxy, high, 1, 2, pt, cam, node, xy, track, counts) == MVBA_OK);  // (the bad edge is beyond n_edges)
  }
  {  // mvba_match_descriptors: the ratio test on exact integers, and the rule that cuts the pair list into chunks
    const double r2 = match_ratio2(0.8);
    CHECK(r2 == 0.8 * 0.8 && match_ratio2(1.0) == 1.0);
    CHECK(match_ambiguous(100, -1, r2) && match_ambiguous(0, -1, 1.0));              // no second: a single candidate passes no ratio test
    CHECK(!match_ambiguous(63, 100, r2) && match_ambiguous(65, 100, r2));            // 0.64...: 63 < 64.0000...01, 65 is not
    CHECK(match_ambiguous(100, 100, 1.0) && !match_ambiguous(99, 100, 1.0));         // equal distances are ambiguous at any ratio
    CHECK(match_ambiguous(0, 0, 1.0) && !match_ambiguous(0, 1, r2));                 // two exact copies; one exact copy
    CHECK(!match_ambiguous(33292799, 33292800, 1.0) && match_ambiguous(33292800, 33292800, 1.0));  // the largest distances there are
    const int64_t kp[5] = {0, 10, 10, 40, 45};  // images of 10, 0, 30, 5 keypoints
    const int32_t pr[10] = {0, 2, 2, 0, 1, 3, 3, 2, 0, 3};
    CHECK(match_chunk_end(kp, pr, 5, 0, false, 1000) == 5 && match_chunk_end(kp, pr, 5, 0, true, 1000) == 5);
    CHECK(match_chunk_end(kp, pr, 5, 0, false, 40) == 3);   // 10 + 30 + 0 queries fit, the 5 of pair 3 do not
    CHECK(match_chunk_end(kp, pr, 5, 0, true, 40) == 1);    // with the reverse direction pair 0 alone has 40 rows
    CHECK(match_chunk_end(kp, pr, 5, 1, true, 1) == 2);     // one pair at least, whatever its size
    CHECK(match_chunk_end(kp, pr, 5, 2, false, 0) == 3 && match_chunk_end(kp, pr, 5, 3, false, 0) == 4);  // (a pair without queries still ends its chunk at budget 0)
    CHECK(match_chunk_end(kp, pr, 5, 5, true, 10) == 5 && match_chunk_end(kp, pr, 0, 0, true, 10) == 0);
    for (int32_t p0 = 0, guard = 0; p0 < 5 && guard < 10; ++guard) {  // the chunks tile the list
      const int32_t p1 = match_chunk_end(kp, pr, 5, p0, true, 35);
      CHECK(p1 > p0 && p1 <= 5);
      p0 = p1;
    }
  }
  {  // its plan and its chunk lists, at budgets of a few dozen rows so that hand-made inputs cross chunk boundaries
    auto check_plan = [&](const std::vector<int64_t> &kp, const std::vector<int32_t> &pr, bool mutual, int64_t budget) {
      const int32_t np = (int32_t)(pr.size() / 2);
      auto size = [&](int im) { return (int)(kp[im + 1] - kp[im]); };
      const MatchPlan pl = match_plan(kp.data(), pr.data(), np, mutual, budget);
      // the cuts are repeated match_chunk_end and cover 0 .. n_pairs exactly
      CHECK(pl.cut.front() == 0 && pl.cut.back() == np && (np > 0 || pl.cut.size() == 1));
      for (size_t c = 0; c + 1 < pl.cut.size(); ++c)
        CHECK(pl.cut[c + 1] > pl.cut[c] && pl.cut[c + 1] == match_chunk_end(kp.data(), pr.data(), np, pl.cut[c], mutual, budget));
      CHECK(pl.max_blocks == (pl.max_q + pl.max_r) / MATCH_TQ + 2 * pl.max_p + 1);
      CHECK(pl.max_dec == (pl.max_q + 255) / 256 && pl.max_sb == (pl.max_q + TRK_SCAN_BLOCK - 1) / TRK_SCAN_BLOCK);
      if (!mutual) CHECK(pl.max_r == 0);
      MatchLists L;  // (one for all chunks, as the entry point keeps it)
      size_t seen_q = 0, seen_r = 0, seen_p = 0;
      for (size_t c = 0; c + 1 < pl.cut.size(); ++c) {
        const int32_t p0 = pl.cut[c], P = pl.cut[c + 1] - p0;
        match_chunk_lists(kp.data(), pr.data(), p0, pl.cut[c + 1], mutual, L);
        CHECK(L.P == P && L.qoff.size() == (size_t)P + 1 && L.roff.size() == (size_t)P + 1 && L.ncand.size() == (size_t)P);
        CHECK(L.qoff[0] == 0 && L.roff[0] == 0 && L.Qc == L.qoff[P]);
        // the bounds the buffers were sized by
        CHECK(L.fwd.size() + L.rev.size() <= pl.max_blocks && (size_t)L.Qc <= pl.max_q && (size_t)L.roff[P] <= pl.max_r && (size_t)P <= pl.max_p);
        seen_q = std::max(seen_q, (size_t)L.Qc), seen_r = std::max(seen_r, (size_t)L.roff[P]), seen_p = std::max(seen_p, (size_t)P);
        if (!mutual) CHECK(L.rev.empty() && std::all_of(L.roff.begin(), L.roff.end(), [](int x) { return x == 0; }));
        // every row of either direction belongs to one block, which asks for the row's own query against the pair's other image
        for (int dir = 0; dir < (mutual ? 2 : 1); ++dir) {
          const std::vector<int> &off = dir ? L.roff : L.qoff;
          std::vector<int> node((size_t)off[P]), c0((size_t)off[P]), nc((size_t)off[P]), hits((size_t)off[P], 0);
          for (int i = 0; i < P; ++i) {
            const int q = pr[2 * (p0 + i) + dir], cnd = pr[2 * (p0 + i) + 1 - dir];
            CHECK(off[i + 1] - off[i] == size(q));
            if (!dir) CHECK(L.ncand[i] == size(cnd));
            for (int j = 0; j < size(q); ++j) node[off[i] + j] = (int)kp[q] + j, c0[off[i] + j] = (int)kp[cnd], nc[off[i] + j] = size(cnd);
          }
          for (const MatchBlock &b : dir ? L.rev : L.fwd) {
            CHECK(b.nq >= 1 && b.nq <= MATCH_TQ && b.out0 >= 0 && b.out0 + b.nq <= off[P]);
            if (!(b.nq >= 1 && b.out0 >= 0 && b.out0 + b.nq <= off[P])) continue;
            for (int j = 0; j < b.nq; ++j) {
              ++hits[b.out0 + j];
              CHECK(node[b.out0 + j] == b.q0 + j && c0[b.out0 + j] == b.c0 && nc[b.out0 + j] == b.nc);
            }
          }
          CHECK(std::all_of(hits.begin(), hits.end(), [](int x) { return x == 1; }));
        }
      }
      CHECK(seen_q == pl.max_q && seen_r == pl.max_r && seen_p == pl.max_p);  // the largest, not merely a bound
      return pl;
    };
    // images of 10, 0, 30, 5, 1, TQ - 1, TQ, TQ + 1 and 300 keypoints; pair (1, 3) has no queries, (0, 1) and (3, 1) no candidates,
    // (8, 2) alone is larger than every small budget
    std::vector<int64_t> kp{0};
    for (int s : {10, 0, 30, 5, 1, MATCH_TQ - 1, MATCH_TQ, MATCH_TQ + 1, 300}) kp.push_back(kp.back() + s);
    const std::vector<int32_t> pr{0, 2, 1, 3, 2, 0, 0, 1, 8, 2, 3, 1, 5, 4, 6, 4, 7, 4, 4, 7, 4, 5, 6, 7, 7, 8, 3, 4, 1, 0};
    for (int mutual = 0; mutual < 2; ++mutual)
      for (int64_t budget : {(int64_t)0, (int64_t)1, (int64_t)35, (int64_t)40, (int64_t)129, (int64_t)300, (int64_t)700, MATCH_CHUNK_QUERIES}) {
        const MatchPlan pl = check_plan(kp, pr, mutual != 0, budget);
        if (budget == MATCH_CHUNK_QUERIES) CHECK(pl.cut.size() == 2 && pl.max_p == pr.size() / 2);
        if (budget == 1) CHECK(pl.cut.size() == pr.size() / 2 + 1 && pl.max_p == 1 && pl.max_q == 300);  // (every pair alone)
      }
    {  // many pairs of one-keypoint images: every job is a block of its own, the 2 max_p term
      std::vector<int64_t> ones{0};
      std::vector<int32_t> chain;
      for (int i = 0; i < 40; ++i) ones.push_back(i + 1);
      for (int i = 0; i + 1 < 40; ++i) chain.insert(chain.end(), {i, i + 1});
      for (int64_t budget : {(int64_t)1, (int64_t)7, (int64_t)1000}) {
        check_plan(ones, chain, false, budget);
        const MatchPlan pl = check_plan(ones, chain, true, budget);
        if (budget == 1000) CHECK(pl.max_p == 39 && pl.max_q == 39 && pl.max_r == 39 && pl.max_blocks == 79);  // 78 blocks in use
      }
    }
    {  // no pairs; and pairs of images that are all empty: one chunk without a query
      const MatchPlan none = check_plan({0, 4, 9}, {}, true, 10);
      CHECK(none.cut.size() == 1 && none.max_q == 0 && none.max_p == 0 && none.max_blocks == 1);
      for (int mutual = 0; mutual < 2; ++mutual) {
        const MatchPlan empty = check_plan({0, 0, 0, 0}, {0, 1, 1, 2, 2, 0}, mutual != 0, 0);
        CHECK(empty.cut.size() == 2 && empty.max_q == 0 && empty.max_r == 0 && empty.max_p == 3 && empty.max_blocks == 7 && empty.max_dec == 0);
      }
    }
    // the grid rule the matcher shares with the track builder, and the "other" slot of a call's timings
    CHECK(trk_grid(0) == 1 && trk_grid(1) == 1 && trk_grid(256) == 1 && trk_grid(257) == 2 && trk_grid((1LL << 31) - 1) == (1u << 23));
    CHECK(lap_rest(10.0, 3.0) == 7.0 && lap_rest(3.0, 10.0) == 0.0 && lap_rest(5.0, 5.0) == 0.0 && lap_rest(0.0, 0.0) == 0.0);
  }
  {  // its checks, with their texts, in the order the entry point looks at its arguments
    const int64_t kp[4] = {0, 2, 2, 5}, down[4] = {0, 3, 2, 5}, off[3] = {1, 2, 3}, big[2] = {0, 1LL << 31}, none[3] = {0, 0, 0};
    const int64_t huge[3] = {0, 1LL << 30, (1LL << 30) + 1};
    const uint8_t desc[5 * 32] = {0};
    const int32_t pr[4] = {0, 2, 2, 0}, high[4] = {0, 2, 3, 0}, low[2] = {0, -1}, self[4] = {0, 2, 2, 2}, twice[4] = {0, 1, 0, 1}, empty[4] = {1, 0, 1, 2};
    int64_t mp[3], counts[MATCH_N_COUNTS], Q = -1;
    int32_t kpp[10], d2[5];
    auto run = [&](int32_t m, const int64_t *kp_, const uint8_t *desc_, int32_t dim, const int32_t *pairs, int32_t np, double ratio, int64_t *mp_,
                   int32_t *kpp_, int32_t *d2_, int64_t *cnt_) { return match_check_args(m, kp_, desc_, dim, pairs, np, ratio, mp_, kpp_, d2_, cnt_, &Q); };
    CHECK(run(3, kp, desc, 32, pr, 2, 0.8, mp, kpp, d2, counts) == MVBA_OK && Q == 5);
    CHECK(run(3, kp, desc, 512, pr, 2, 0.0, mp, kpp, d2, counts) == MVBA_OK && run(3, kp, desc, 16, pr, 2, 1.0, mp, kpp, d2, counts) == MVBA_OK);
    CHECK(run(3, kp, desc, 32, nullptr, 0, 0.8, mp, kpp, d2, counts) == MVBA_OK && Q == 0);  // no pairs: the pointer is not looked at
    CHECK(run(3, kp, desc, 32, empty, 2, 0.8, mp, kpp, d2, counts) == MVBA_OK && Q == 0);    // every query image is empty
    CHECK(run(2, none, nullptr, 128, nullptr, 0, 0.8, mp, kpp, d2, counts) == MVBA_OK);      // no keypoints: desc is not looked at
    CHECK(run(3, nullptr, desc, 32, pr, 2, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "null argument: kp_ptr (argument 2)");
    CHECK(run(3, kp, desc, 32, pr, 2, 0.8, nullptr, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "null argument: match_ptr (argument 10)");
    CHECK(run(3, kp, desc, 32, pr, 2, 0.8, mp, nullptr, d2, counts) == MVBA_ERR_BADARG && g_err == "null argument: kp_pairs (argument 11)");
    CHECK(run(3, kp, desc, 32, pr, 2, 0.8, mp, kpp, nullptr, counts) == MVBA_ERR_BADARG && g_err == "null argument: dist2 (argument 12)");
    CHECK(run(3, kp, desc, 32, pr, 2, 0.8, mp, kpp, d2, nullptr) == MVBA_ERR_BADARG && g_err == "null argument: counts (argument 16)");
    CHECK(run(3, kp, nullptr, 32, pr, 2, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "null argument: desc (argument 3) with 5 keypoints");
    CHECK(run(3, kp, desc, 32, nullptr, 2, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "null argument: pairs (argument 5) with n_pairs = 2");
    CHECK(run(3, kp, desc, 32, pr, -1, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "n_pairs = -1: negative size");
    CHECK(run(0, kp, desc, 32, pr, 2, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "n_images = 0 must be at least 1");
    CHECK(run(2, off, desc, 32, pr, 0, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "kp_ptr[0] = 1 must be 0");
    CHECK(run(3, down, desc, 32, pr, 2, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "kp_ptr is not ascending: kp_ptr[2] = 2 after 3");
    CHECK(run(1, big, desc, 32, pr, 0, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "n_nodes = kp_ptr[n_images] = 2147483648 must be < 2^31");
    for (int32_t dim : {0, 8, 24, 520, 528, -16}) {
      CHECK(run(3, kp, desc, dim, pr, 2, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG);
      CHECK(g_err == "dim = " + std::to_string(dim) + " must be a multiple of 16 in 16 .. 512");
    }
    CHECK(run(3, kp, desc, 32, pr, 2, -0.1, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "ratio = -0.100000 must be in (0, 1], or 0 for no ratio test");
    CHECK(run(3, kp, desc, 32, pr, 2, 1.5, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "ratio = 1.500000 must be in (0, 1], or 0 for no ratio test");
    CHECK(run(3, kp, desc, 32, pr, 2, std::numeric_limits<double>::quiet_NaN(), mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err.find("nan must be in") != std::string::npos);
    CHECK(run(3, kp, desc, 32, high, 2, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "pairs[1][0] = 3: image index out of range, n_images = 3");
    CHECK(run(3, kp, desc, 32, low, 1, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "pairs[0][1] = -1: image index out of range, n_images = 3");
    CHECK(run(3, kp, desc, 32, self, 2, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "pairs[1] = (2, 2): an image is not matched with itself");
    CHECK(run(2, huge, desc, 32, twice, 2, 0.8, mp, kpp, d2, counts) == MVBA_ERR_BADARG && g_err == "Q = 2147483648 queries up to pair 1: the sum over the pairs must be < 2^31");
    CHECK(run(2, huge, desc, 32, twice, 1, 0.8, mp, kpp, d2, counts) == MVBA_OK && Q == (1LL << 30));
  }
  {  // the compact record expanded for mvba_debug_read (expand_compact_record) against obs_math's own rows: slots 0..3 and the
     // residual pass through, J_omega = (row of J_X) x (X - t) to 1e-14 of the largest entry; a unit case by hand
    const double f0 = 600.0, th = 0.3;
    const double cam[CAM_IN] = {1.1 * f0, 7.0, -5.0, 0.4, -0.2, -3.0, cos(th), 0.0, sin(th), 0.0, 1.0, 0.0, -sin(th), 0.0, cos(th)};
    alignas(16) double c18[CAM_LDS];
    expand_cam(cam, f0, c18);
    const double X[3] = {0.7, -0.4, 2.5};
    ObsJ J;
    obs_math(X[0], X[1], X[2], c18, 31.0, -12.0, f0, J);
    double c8[8], e2[2] = {J.e0, J.e1}, full[16];
    for (int i = 0; i < 3; ++i) { c8[2 * i] = J.jx[0][i]; c8[2 * i + 1] = J.jx[1][i]; }
    c8[6] = J.jc[0][0]; c8[7] = J.jc[1][0];
    expand_compact_record(c8, e2, X, cam + 3, full);
    for (int i = 0; i < 8; ++i) CHECK(full[i] == c8[i]);
    CHECK(full[14] == J.e0 && full[15] == J.e1);
    double big = 0.0;
    for (int rr = 0; rr < 2; ++rr) for (int i = 6; i < 9; ++i) big = std::max(big, std::fabs(J.jc[rr][i]));
    CHECK(big > 0.0);
    for (int rr = 0; rr < 2; ++rr) for (int i = 0; i < 3; ++i) CHECK(std::fabs(full[8 + 2 * i + rr] - J.jc[rr][6 + i]) <= 1e-14 * big);
    const double jx[8] = {1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0}, zero[3] = {0.0, 0.0, 0.0}, d[3] = {2.0, 3.0, 5.0};
    expand_compact_record(jx, e2, d, zero, full);  // rows e_x, e_y; d = (2, 3, 5): e_x x d = (0, -5, 3), e_y x d = (5, 0, -2)
    CHECK(full[8] == 0.0 && full[10] == -5.0 && full[12] == 3.0 && full[9] == 5.0 && full[11] == 0.0 && full[13] == -2.0);
  }
  // ---------------------------------------------------------------- the BA engine's host logic (mvba_engine_host.h)
  auto default_map = [](int m, int axis) {
    std::vector<int32_t> col(9 * m);
    for (int g = 0, j = 0; g < 9 * m; ++g) col[g] = is_gauge_slot(g, axis) ? -1 : j++;
    return col;
  };
  auto transpose_ok = [](const std::vector<int32_t> &col, int n_free, const ParameterMap &pm) {  // ptr / mem against a transpose written here
    if ((int)pm.ptr.size() != n_free + 1 || pm.ptr[0] != 0) return false;
    for (int j = 0; j < n_free; ++j) {
      std::vector<int> slots;
      for (int g = 0; g < (int)col.size(); ++g)
        if (col[g] == j) slots.push_back(g);
      if (pm.ptr[j + 1] - pm.ptr[j] != (int)slots.size()) return false;
      for (size_t q = 0; q < slots.size(); ++q)
        if (pm.mem[pm.ptr[j] + q] != slots[q]) return false;
    }
    return (int)pm.mem.size() == std::max(pm.ptr[n_free], 1);
  };
  // every f of m cameras one unknown (the last), everything else as the default map numbers it
  auto shared_f_map = [&](int m, int axis, int &n_free) {
    std::vector<int32_t> col(9 * m);
    int j = 0;
    for (int g = 0; g < 9 * m; ++g) col[g] = (is_gauge_slot(g, axis) || g % 9 == 0) ? -1 : j++;
    for (int k = 0; k < m; ++k) col[9 * k] = j;
    n_free = j + 1;
    return col;
  };
  {  // parameter maps at m = 3: 27 slots, D = 20
    const int m = 3, D = 20;
    for (int axis = 0; axis < 3; ++axis) {
      ParameterMap pm;
      std::vector<int32_t> col = default_map(m, axis);
      CHECK(is_gauge_slot(3, axis) && is_gauge_slot(8, axis) && is_gauge_slot(12 + axis, axis) && !is_gauge_slot(2, axis) && !is_gauge_slot(9, axis) &&
            !is_gauge_slot(12 + (axis + 1) % 3, axis));
      CHECK(build_parameter_map(col.data(), m, axis, D, D, pm) == MVBA_OK && pm.is_default);  // spelled out: recognised as the default
      std::vector<int32_t> none(27, -1);  // everything held
      CHECK(build_parameter_map(none.data(), m, axis, 0, D, pm) == MVBA_OK && !pm.is_default);
      CHECK(pm.ptr.size() == 1 && pm.ptr[0] == 0 && pm.mem.size() == 1 && pm.U == 0 && pm.pairs.empty() && pm.nblk == 1);
      {  // f of cameras 0 and 2 tied, as the last unknown
        std::vector<int32_t> c(27);
        int j = 0;
        for (int g = 0; g < 27; ++g) c[g] = (is_gauge_slot(g, axis) || g == 0 || g == 18) ? -1 : j++;
        c[0] = c[18] = j;
        const int n_free = j + 1;
        CHECK(n_free == D - 1);
        CHECK(build_parameter_map(c.data(), m, axis, n_free, D, pm) == MVBA_OK && !pm.is_default);
        CHECK(pm.U == n_free - 1 && pm.pairs.size() == 1 && pm.pairs[0].x == n_free - 1 && pm.pairs[0].y == n_free - 1 && pm.nblk == 1);
        CHECK(transpose_ok(c, n_free, pm));
        CHECK(pm.ptr[n_free] == D && pm.mem[pm.ptr[n_free - 1]] == 0 && pm.mem[pm.ptr[n_free - 1] + 1] == 18);
      }
      {  // a tied unknown (u of cameras 1 and 2) numbered 2, before untied ones: U stops at it
        std::vector<int32_t> c(27);
        int j = 0;
        for (int g = 0; g < 27; ++g) c[g] = is_gauge_slot(g, axis) ? -1 : (g == 19 ? -2 : j++);
        c[19] = c[10];
        CHECK(c[10] > 2);
        for (int g = 0; g < 27; ++g)  // renumber: unknown c[10] <-> unknown 2
          if (c[g] == c[10] && g != 10 && g != 19) c[g] = -3;
        const int tied = c[10];
        for (int g = 0; g < 27; ++g) c[g] = c[g] == 2 ? tied : (c[g] == tied ? 2 : c[g]);
        CHECK(c[10] == 2 && c[19] == 2);
        CHECK(build_parameter_map(c.data(), m, axis, j, D, pm) == MVBA_OK && pm.U == 2 && pm.pairs.size() == 1 && pm.pairs[0].x == 2 && pm.nblk == 1);
        CHECK(transpose_ok(c, j, pm));
      }
      // the refusals, with their texts
      g_err.clear();
      CHECK(build_parameter_map(col.data(), m, axis, D + 1, D, pm) == MVBA_ERR_BADARG && g_err == "mvba_set_parameter_map: n_free = 21 must be in 0 .. 9 n_images - 7 = 20");
      CHECK(build_parameter_map(col.data(), m, axis, -1, D, pm) == MVBA_ERR_BADARG && g_err == "mvba_set_parameter_map: n_free = -1 must be in 0 .. 9 n_images - 7 = 20");
      std::vector<int32_t> bad = col;
      bad[0] = D;
      CHECK(build_parameter_map(bad.data(), m, axis, D, D, pm) == MVBA_ERR_BADARG && g_err == "mvba_set_parameter_map: col[0] = 20 is neither -1 nor below n_free = 20");
      bad[0] = -2;
      CHECK(build_parameter_map(bad.data(), m, axis, D, D, pm) == MVBA_ERR_BADARG && g_err == "mvba_set_parameter_map: col[0] = -2 is neither -1 nor below n_free = 20");
      bad = col; bad[3] = 0;
      CHECK(build_parameter_map(bad.data(), m, axis, D, D, pm) == MVBA_ERR_BADARG && g_err == "mvba_set_parameter_map: col[3] is a gauge slot and must be -1");
      bad = col; bad[12 + axis] = 0;
      CHECK(build_parameter_map(bad.data(), m, axis, D, D, pm) == MVBA_ERR_BADARG &&
            g_err == "mvba_set_parameter_map: col[" + std::to_string(12 + axis) + "] is a gauge slot and must be -1");
      bad = col; bad[1] = bad[0];  // f tied to u
      CHECK(build_parameter_map(bad.data(), m, axis, D, D, pm) == MVBA_ERR_BADARG &&
            g_err == "mvba_set_parameter_map: col[1] ties slot 1 to slot 0 (unknown 0): only the same intrinsic parameter (f, u or v) of different cameras can be tied");
      bad = col; bad[24] = bad[15];  // an omega of camera 2 tied to the same omega of camera 1: not an intrinsic
      CHECK(build_parameter_map(bad.data(), m, axis, D, D, pm) == MVBA_ERR_BADARG &&
            g_err == "mvba_set_parameter_map: col[24] ties slot 24 to slot 15 (unknown " + std::to_string(col[15]) +
                         "): only the same intrinsic parameter (f, u or v) of different cameras can be tied");
      bad = col; bad[0] = -1;
      CHECK(build_parameter_map(bad.data(), m, axis, D, D, pm) == MVBA_ERR_BADARG && g_err == "mvba_set_parameter_map: unknown 0 has no parameter slot");
    }
  }
  for (int m : {9, 513}) {  // all f shared: nblk = 2 at nine members, 64 (the cap) at 513
    int n_free = 0;
    const std::vector<int32_t> col = shared_f_map(m, 1, n_free);
    ParameterMap pm;
    CHECK(n_free == 9 * m - 7 - m + 1);
    CHECK(build_parameter_map(col.data(), m, 1, n_free, 9 * m - 7, pm) == MVBA_OK && !pm.is_default);
    CHECK(pm.nblk == (m == 9 ? 2 : 64) && pm.U == n_free - 1 && pm.pairs.size() == 1 && pm.ptr[n_free] - pm.ptr[n_free - 1] == m);
    CHECK(transpose_ok(col, n_free, pm));
  }
  {  // the residual of the reduced system: packed strips from a dense SPD matrix, x from a plain Gaussian elimination
    auto solve = [](std::vector<double> A, std::vector<double> b, int n) {  // partial pivoting, A row-major n x n
      for (int c = 0; c < n; ++c) {
        int piv = c;
        for (int r = c + 1; r < n; ++r)
          if (std::fabs(A[(size_t)r * n + c]) > std::fabs(A[(size_t)piv * n + c])) piv = r;
        for (int j = 0; j < n; ++j) std::swap(A[(size_t)c * n + j], A[(size_t)piv * n + j]);
        std::swap(b[c], b[piv]);
        for (int r = c + 1; r < n; ++r) {
          const double f = A[(size_t)r * n + c] / A[(size_t)c * n + c];
          for (int j = c; j < n; ++j) A[(size_t)r * n + j] -= f * A[(size_t)c * n + j];
          b[r] -= f * b[c];
        }
      }
      for (int r = n - 1; r >= 0; --r) {
        for (int j = r + 1; j < n; ++j) b[r] -= A[(size_t)r * n + j] * b[j];
        b[r] /= A[(size_t)r * n + r];
      }
      return b;
    };
    for (int m : {2, 3})
      for (int axis = 0; axis < 3; ++axis) {
        const int n9 = 9 * m;
        unsigned long long seed = 12345 + 7 * m + axis;
        auto rnd = [&]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / (double)(1ULL << 53) - 0.5; };
        std::vector<double> B((size_t)n9 * n9), M((size_t)n9 * n9, 0.0), b(n9);
        for (double &v : B) v = rnd();
        for (int i = 0; i < n9; ++i)
          for (int j = 0; j < n9; ++j) {
            for (int k = 0; k < n9; ++k) M[(size_t)i * n9 + j] += B[(size_t)i * n9 + k] * B[(size_t)j * n9 + k];
            if (i == j) M[(size_t)i * n9 + j] += 1.0;
          }
        for (double &v : b) v = rnd();
        const size_t nA = strip_offset(m, m);
        std::vector<double> Ab(nA + n9);
        for (int k = 0; k < m; ++k)
          for (int i = 0; i < 9; ++i)
            for (int c = 0; c < 9 * (m - k); ++c) Ab[strip_offset(k, m) + (size_t)i * 9 * (m - k) + c] = M[(size_t)(9 * k + i) * n9 + 9 * k + c];
        for (int g = 0; g < n9; ++g) Ab[nA + g] = is_gauge_slot(g, axis) ? 1e30 : b[g];  // the gauge rows must not enter
        // the default form: the system over the kept slots
        std::vector<int> kept;
        for (int g = 0; g < n9; ++g)
          if (!is_gauge_slot(g, axis)) kept.push_back(g);
        const int D = (int)kept.size();
        CHECK(D == n9 - 7);
        std::vector<double> Mk((size_t)D * D), bk(D);
        for (int i = 0; i < D; ++i) {
          bk[i] = b[kept[i]];
          for (int j = 0; j < D; ++j) Mk[(size_t)i * D + j] = M[(size_t)kept[i] * n9 + kept[j]];
        }
        const std::vector<double> xk = solve(Mk, bk, D);
        std::vector<double> x(n9, 0.0);
        for (int i = 0; i < D; ++i) x[kept[i]] = xk[i];
        double worst = reduced_system_residual(Ab.data(), x.data(), m, axis, nullptr, nullptr, D);
        CHECK(worst < 1e-12);
        x[kept[D / 2]] += 1e-3;
        worst = reduced_system_residual(Ab.data(), x.data(), m, axis, nullptr, nullptr, D);
        CHECK(worst > 1e-8);
        if (m < 3) continue;
        // the mapped form with one tie: f of cameras 0 and 2 one unknown, M' = P^T M P, b' = P^T b, dxi = P x'
        std::vector<int32_t> col(n9);
        int j = 0;
        for (int g = 0; g < n9; ++g) col[g] = (is_gauge_slot(g, axis) || g == 0 || g == 18) ? -1 : j++;
        col[0] = col[18] = j;
        const int n_free = j + 1;
        ParameterMap pm;
        CHECK(build_parameter_map(col.data(), m, axis, n_free, D, pm) == MVBA_OK);
        std::vector<double> Mp((size_t)n_free * n_free, 0.0), bp(n_free, 0.0);
        for (int g = 0; g < n9; ++g) {
          if (col[g] < 0) continue;
          bp[col[g]] += b[g];
          for (int g2 = 0; g2 < n9; ++g2)
            if (col[g2] >= 0) Mp[(size_t)col[g] * n_free + col[g2]] += M[(size_t)g * n9 + g2];
        }
        const std::vector<double> xp = solve(Mp, bp, n_free);
        std::vector<double> dxi(n9, 0.0);
        for (int g = 0; g < n9; ++g)
          if (col[g] >= 0) dxi[g] = xp[col[g]];
        CHECK(dxi[0] == dxi[18]);
        worst = reduced_system_residual(Ab.data(), dxi.data(), m, axis, pm.ptr.data(), pm.mem.data(), n_free);
        CHECK(worst < 1e-12);
        dxi[1] += 1e-3;
        worst = reduced_system_residual(Ab.data(), dxi.data(), m, axis, pm.ptr.data(), pm.mem.data(), n_free);
        CHECK(worst > 1e-8);
      }
  }
  {  // the packed strips expanded: diagonal blocks as stored (they are not symmetric here), the others mirrored
    const int m = 3, n9 = 27;
    std::vector<double> pk(strip_offset(m, m)), out((size_t)n9 * n9, -1.0);
    CHECK(pk.size() == 486);
    for (size_t i = 0; i < pk.size(); ++i) pk[i] = 1.0 + (double)i;
    expand_packed_A(pk.data(), m, out.data());
    for (int k = 0; k < m; ++k)
      for (int l = k; l < m; ++l)
        for (int i = 0; i < 9; ++i)
          for (int jj = 0; jj < 9; ++jj) {
            const double stored = pk[strip_offset(k, m) + (size_t)i * 9 * (m - k) + 9 * (l - k) + jj];
            CHECK(out[(size_t)(9 * k + i) * n9 + 9 * l + jj] == stored);
            if (l > k) CHECK(out[(size_t)(9 * l + jj) * n9 + 9 * k + i] == stored);
          }
    CHECK(out[1] != out[n9]);  // (0, 1) and (1, 0) of the first diagonal block: both halves kept as computed
  }
  {  // a record as the C interface's rows
    double q[16], e[2], jx[6], jc[18];
    for (int i = 0; i < 16; ++i) q[i] = 1.0 + i;
    record_to_residual(q, e);
    CHECK(e[0] == 15.0 && e[1] == 16.0);
    record_to_JX(q, jx);
    const double want_jx[6] = {1, 3, 5, 2, 4, 6};
    for (int i = 0; i < 6; ++i) CHECK(jx[i] == want_jx[i]);
    for (double f0 : {1.0, 600.0})
      for (double sqw : {1.0, 0.5}) {  // cu = 1 / f0, and sqrt(w) / f0 with w = 1 / 4
        const double cu = sqw == 1.0 ? 1.0 / f0 : sqw / f0;
        record_to_JC(q, cu, jc);
        const double want[18] = {7, cu, 0, -1, -3, -5, 9, 11, 13, 8, 0, cu, -2, -4, -6, 10, 12, 14};
        for (int i = 0; i < 18; ++i) CHECK(jc[i] == want[i]);
        for (int rr = 0; rr < 2; ++rr) for (int i = 0; i < 3; ++i) CHECK(jc[9 * rr + 3 + i] == -jx[3 * rr + i]);  // the -J_X columns
      }
  }
  {  // cam15: a round trip at m = 2, all 15 entries of a row distinct
    const int m = 2;
    double f[2], u[4], t[6], R[18], cam[2 * CAM_IN], f2[2], u2[4], t2[6], R2[18];
    for (int k = 0; k < m; ++k) {
      f[k] = 100 + k;
      for (int i = 0; i < 2; ++i) u[2 * k + i] = 200 + 2 * k + i;
      for (int i = 0; i < 3; ++i) t[3 * k + i] = 300 + 3 * k + i;
      for (int i = 0; i < 9; ++i) R[9 * k + i] = 400 + 9 * k + i;
    }
    pack_cam15(m, f, u, t, R, cam);
    for (int k = 0; k < m; ++k) {
      const double *c = cam + CAM_IN * k;
      CHECK(c[0] == f[k] && c[1] == u[2 * k] && c[2] == u[2 * k + 1] && c[3] == t[3 * k] && c[5] == t[3 * k + 2] && c[6] == R[9 * k] && c[14] == R[9 * k + 8]);
    }
    unpack_cam15(cam, m, f2, u2, t2, R2);
    CHECK(!memcmp(f, f2, sizeof f) && !memcmp(u, u2, sizeof u) && !memcmp(t, t2, sizeof t) && !memcmp(R, R2, sizeof R));
  }
  {  // the width rules.  Table bytes: 8 * 28 * m for K5 (camera row + update row), 8 * 18 * m for the cost pass
    auto k5_bytes = [](int m) { return sizeof(double) * (size_t)(CAM_LDS + DXI_LDS) * m; };
    auto cost_threads = [](int m) { return std::min(512, table_block_threads(sizeof(double) * (size_t)CAM_LDS * m)); };
    CHECK(k5_bytes(182) == 40768 && k5_bytes(183) == 40992 && k5_bytes(365) == 81760 && k5_bytes(366) == 81984);
    CHECK(table_block_threads(k5_bytes(182)) == 256 && table_block_threads(k5_bytes(183)) == 512);
    CHECK(table_block_threads(k5_bytes(365)) == 512 && table_block_threads(k5_bytes(366)) == 1024);
    CHECK(table_block_threads(40 * 1024) == 256 && table_block_threads(80 * 1024) == 512 && table_block_threads(0) == 256);
    CHECK(cost_threads(284) == 256 && cost_threads(285) == 512 && cost_threads(646) == 512);
    CHECK(k5_lanes(40.0) == 2 && k5_lanes(std::nextafter(40.0, 41.0)) == 4 && k5_lanes(100.0) == 4 && k5_lanes(std::nextafter(100.0, 101.0)) == 8 && k5_lanes(1.0) == 2);
    CHECK(cov_lanes(12.0) == 8 && cov_lanes(std::nextafter(12.0, 13.0)) == 16 && cov_lanes(24.0) == 16 && cov_lanes(std::nextafter(24.0, 25.0)) == 32);
    CHECK(cov_lanes(48.0) == 32 && cov_lanes(std::nextafter(48.0, 49.0)) == 64 && cov_lanes(0.0) == 8);
    auto in = [](auto &dom, int v) { return std::find(std::begin(dom), std::end(dom), v) != std::end(dom); };  // the domain beside the rule
    for (double d : {1.0, 40.0, 41.0, 100.0, 101.0, 1e6}) CHECK(in(K5_LANES, k5_lanes(d)));
    for (size_t by : {(size_t)0, (size_t)40961, (size_t)81921, (size_t)160 * 1024}) CHECK(in(TABLE_BLOCK_THREADS, table_block_threads(by)));
    for (double pr : {0.0, 13.0, 25.0, 49.0, 1e6}) CHECK(in(COV_LANES, cov_lanes(pr)));
    CHECK(std::size(K5_LANES) == 3 && std::size(TABLE_BLOCK_THREADS) == 3 && std::size(COV_LANES) == 4);
  }
  {  // the lane form's packed index row: (k, l, a) -> two words -> (k, l, a) at every edge of the three fields
    const int ROW = (int)LANE_IDX_MAX_ROW, OFF = (int)LANE_IDX_MAX_OFF;
    CHECK(LANE_IDX_ROW_BITS == 25 && LANE_IDX_OFF_BITS == 14 && ROW == (1 << 25) - 1 && OFF == 16383);
    auto round_trip = [](int k, int l, int a) {
      int k2 = -1, l2 = -1, a2 = -1;
      const LaneIdx p = lane_idx_pack(k, l, a);
      lane_idx_unpack(p, k2, l2, a2);
      return k2 == k && l2 == l && a2 == a && lane_idx_k(p.w0) == k && lane_idx_l(p.w0, p.w1) == l && lane_idx_a(p.w1) == a;
    };
    const int ks[] = {0, 1, 127, 128, (1 << 24) + 5, ROW - OFF, ROW - 1, ROW}, as[] = {0, 1, 77, 1 << 24, ROW - 1, ROW};
    const int ds[] = {0, 1, 63, 64, 79, 127, 128, 129, 255, 256, 8191, 8192, OFF - 1, OFF};
    for (int k : ks)
      for (int d : ds)
        for (int a : as)
          if ((long long)k + d <= ROW) CHECK(round_trip(k, k + d, a));
    CHECK(round_trip(ROW - OFF, ROW, ROW));  // the largest record index, offset and point row at once
    {  // the padding item (the range's first record twice, the all-zero point row N) and a diagonal item (l = k)
      const int N = 1234567;
      const LaneIdx pad = lane_idx_pack(0, 0, N), dg = lane_idx_pack(4711, 4711, 42);
      CHECK(pad.w0 == 0u && pad.w1 == (unsigned)N && round_trip(0, 0, N) && round_trip(0, 0, ROW));
      CHECK(dg.w0 == 4711u && dg.w1 == 42u && lane_idx_l(dg.w0, dg.w1) == lane_idx_k(dg.w0));
    }
    // the fields do not run into each other: the offset's two halves alone, and all ones
    CHECK(lane_idx_pack(0, 127, 0).w0 == 127u << 25 && lane_idx_pack(0, 127, 0).w1 == 0u);
    CHECK(lane_idx_pack(0, 128, 0).w0 == 0u && lane_idx_pack(0, 128, 0).w1 == 1u << 25);
    CHECK(lane_idx_pack(ROW - OFF, ROW, ROW).w1 == 0xffffffffu);
    static_assert(lane_idx_l(lane_idx_pack(5, 300, 9).w0, lane_idx_pack(5, 300, 9).w1) == 300, "constexpr on the host and in the kernels");
    // what decide_schur_form asks before it takes the lane form: the byte-offset guards' largest scene fits, one more does not
    const long long NMAX = (1LL << 32) / 128 - 2;  // the largest N with (N + 1) * 128 < 2^32
    CHECK((NMAX + 1) * 128 < (1LL << 32) && (NMAX + 2) * 128 >= (1LL << 32));
    CHECK(lane_idx_fits(NMAX, NMAX, 16384) && !lane_idx_fits(NMAX, NMAX, 16385) && lane_idx_fits(0, 0, 0) && lane_idx_fits(10, 20, 1));
    CHECK(!lane_idx_fits(ROW + 1, 10, 2) && !lane_idx_fits(10, ROW + 2, 2) && lane_idx_fits(ROW, ROW + 1, 2));
  }
  {  // the lane form's range count: the largest nR with nR * waves <= places, capped at 8 * (1 .. 8) by the typical list, at least 1
    const long long T = 10000;  // (the typical off-diagonal list of 1 M points at 10 %: the cap is 64)
    CHECK(lane_ranges(1024, 95, T, 0) == 10 && lane_ranges(768, 95, T, 0) == 8);  // 100 cameras: four places per CU, three
    CHECK(lane_ranges(1024, 78, T, 0) == 13 && lane_ranges(1024, 63, T, 0) == 16 && lane_ranges(1024, 96, T, 0) == 10);
    CHECK(lane_ranges(1024, 1024, T, 0) == 1 && lane_ranges(1024, 1025, T, 0) == 1 && lane_ranges(1024, 513, T, 0) == 1 && lane_ranges(1024, 512, T, 0) == 2);
    CHECK(lane_ranges(1000, 96, T, 0) == 10 && lane_ranges(959, 96, T, 0) == 9);  // places that the waves of a range do not divide
    CHECK(lane_ranges(1024, 1, T, 0) == 64 && lane_ranges(1024, 9, 1LL << 40, 0) == 64 && lane_ranges(1024, 9, 1024, 0) == 16 && lane_ranges(1024, 9, 1023, 0) == 8);
    CHECK(lane_ranges(1024, 9, 0, 0) == 8 && lane_ranges(1024, 200, 0, 0) == 5 && lane_ranges(0, 9, T, 0) == 1 && lane_ranges(1024, 0, T, 0) == 64);
    CHECK(lane_ranges(1024, 95, T, 1) == 1 && lane_ranges(1024, 95, T, 3) == 3 && lane_ranges(1024, 95, T, 11) == 11 && lane_ranges(768, 95, 0, 64) == 64);
    CHECK(lane_ranges(1024, 95, T, 65) == LANE_MAX_RANGES && lane_ranges(1024, 95, T, 1 << 30) == LANE_MAX_RANGES);
  }
  {  // block -> wave of the lane form's launch: a permutation of the waves; a range among the first 8 (nR / 8) keeps to XCD r % 8, the
     // surplus ranges' waves are spread evenly; the identity for a multiple of 8 and below 8
    for (int nR : {1, 3, 7, 8, 9, 10, 11, 15, 16, 17, 23, 64})
      for (int rw : {1, 2, 9, 95, 96}) {
        const int T = nR * rw, q = nR / 8;
        std::vector<int> seen(T, 0), surplus(8, 0);
        bool home_ok = true, same = true, order = true;
        std::vector<int> last_w(nR, -1);
        for (int B = 0; B < T; ++B) {
          const int b = lane_wave_of_block(B, nR, rw);
          if (b < 0 || b >= T) { home_ok = false; continue; }
          ++seen[b];
          const int r = b % nR, w = b / nR;
          if (r < 8 * q) home_ok = home_ok && B % 8 == r % 8;
          else ++surplus[B % 8];
          same = same && b == B;
          order = order && w > last_w[r];  // a range's waves are dispatched in wave order (the diagonal lists first)
          last_w[r] = w;
        }
        CHECK(std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; }));
        CHECK(home_ok && order);
        CHECK(*std::max_element(surplus.begin(), surplus.end()) - *std::min_element(surplus.begin(), surplus.end()) <= 1);
        CHECK(same || (nR % 8 != 0 && nR > 8));
      }
  }
  if (failures) return 1;
  std::printf("host_check ok\n");
  return 0;
}
