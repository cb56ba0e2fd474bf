// The BA engine's host logic with no HIP call in it: the gauge predicate, the checks and tables of a parameter map, the residual of
// the reduced system (MVBA_CHECK_SOLVE), the packed strips and the records as mvba_debug_read hands them out, the cam15 row, the
// lane form's packed index row and range count, and the width rules of K5, the cost pass and the covariance's point pass.  Plain functions over pointers and std::vectors, none
// takes an mvba_handle: csrc/host_check.cpp runs them on hand-made inputs under the host sanitizers.
//
// Needs mvba_common.h alone (fail, strip_offset, CAM_IN).  Included by mvba.hip before the engine (mvba_engine.h and the headers
// after it use it) and by host_check.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

#include "mvba_common.h"

namespace mvba {

// the seven parameters the gauge removes: camera 0's t and R, one component of camera 1's t (the host's view of keep_index)
inline bool is_gauge_slot(long long g, int axis) { return (g >= 3 && g <= 8) || g == 12 + axis; }

// ------------------------------------------------------------------ parameter maps (mvba_set_parameter_map)
// What a map `col` [9 m] (slot -> unknown, or -1: held) becomes: the CSR transpose (unknown j's slots mem[ptr[j] .. ptr[j + 1]),
// ascending), the first U unknowns with one slot each, the (a, b <= a) pairs of tied unknowns and the workgroups that share one
// pair's sum: eight of the row's members each, 64 at most.  is_default: the map spells out the default one, nothing else is filled.
struct ParameterMap {
  bool is_default = false;
  std::vector<int> ptr, mem;
  std::vector<int2> pairs;
  int U = 0, nblk = 1;
};

inline int build_parameter_map(const int32_t *col, int m, int axis, int n_free, int D, ParameterMap &out) {
  const int n9 = 9 * m;
  if (n_free < 0 || n_free > D)
    return fail(MVBA_ERR_BADARG, "mvba_set_parameter_map: n_free = " + std::to_string(n_free) + " must be in 0 .. 9 n_images - 7 = " + std::to_string(D));
  std::vector<int> cnt(n_free + 1, 0), first(n_free, -1);
  for (int g = 0; g < n9; ++g) {
    const int j = col[g];
    if (j < -1 || j >= n_free)
      return fail(MVBA_ERR_BADARG, "mvba_set_parameter_map: col[" + std::to_string(g) + "] = " + std::to_string(j) + " is neither -1 nor below n_free = " + std::to_string(n_free));
    if (j >= 0 && is_gauge_slot(g, axis))
      return fail(MVBA_ERR_BADARG, "mvba_set_parameter_map: col[" + std::to_string(g) + "] is a gauge slot and must be -1");
    if (j < 0) continue;
    if (first[j] < 0) first[j] = g;
    else if (g % 9 != first[j] % 9 || g % 9 > 2)
      return fail(MVBA_ERR_BADARG, "mvba_set_parameter_map: col[" + std::to_string(g) + "] ties slot " + std::to_string(g) + " to slot " + std::to_string(first[j]) +
                                       " (unknown " + std::to_string(j) + "): only the same intrinsic parameter (f, u or v) of different cameras can be tied");
    ++cnt[j];
  }
  for (int j = 0; j < n_free; ++j)
    if (!cnt[j]) return fail(MVBA_ERR_BADARG, "mvba_set_parameter_map: unknown " + std::to_string(j) + " has no parameter slot");
  out = ParameterMap();
  out.is_default = n_free == D;
  for (int g = 0, j = 0; out.is_default && g < n9; ++g) out.is_default = col[g] == (is_gauge_slot(g, axis) ? -1 : j++);
  if (out.is_default) return MVBA_OK;
  out.ptr.assign(n_free + 1, 0);
  for (int j = 0; j < n_free; ++j) out.ptr[j + 1] = out.ptr[j] + cnt[j];
  out.mem.resize(std::max(out.ptr[n_free], 1));
  {
    std::vector<int> fill(out.ptr.begin(), out.ptr.end() - 1);
    for (int g = 0; g < n9; ++g)
      if (col[g] >= 0) out.mem[fill[col[g]]++] = g;  // ascending g within an unknown
  }
  while (out.U < n_free && cnt[out.U] == 1) ++out.U;
  int max_cnt = 1;
  std::vector<int> tied;
  for (int j = 0; j < n_free; ++j)
    if (cnt[j] > 1) { tied.push_back(j); max_cnt = std::max(max_cnt, cnt[j]); }
  for (size_t a = 0; a < tied.size(); ++a)
    for (size_t b = 0; b <= a; ++b) out.pairs.push_back(make_int2(tied[a], tied[b]));
  out.nblk = std::min(64, (max_cnt + 7) / 8);
  return MVBA_OK;
}

// ------------------------------------------------------------------ MVBA_CHECK_SOLVE
// The relative residual of the reduced system, worst row: b - A x over the kept parameters, from the packed [A|b] (`Ab`:
// strip_offset(m, m) + 9 m doubles) and the full-length x = dxi, in plain loops.  With a map (map_ptr != null; n_free unknowns) it
// is the mapped system's P^T (b - A P x): x is dxi = P x, the rows are summed over an unknown's members.
inline double reduced_system_residual(const double *Ab, const double *x, int m, int axis, const int *map_ptr, const int *map_mem, int n_free) {
  const size_t n9 = 9 * (size_t)m, nA = strip_offset(m, m);
  std::vector<double> r(n9, 0.0), an(n9, 0.0);  // r = A x, an = |A| |x|  (rows of the full symmetric matrix from the packed upper strips)
  for (int k = 0; k < m; ++k) {
    const double *Ak = Ab + strip_offset(k, m);
    const int Wk = 9 * (m - k);
    for (int i = 0; i < 9; ++i)
      for (int c = 0; c < Wk; ++c) {
        const size_t gi = 9 * (size_t)k + i, gj = 9 * (size_t)k + c;
        const double a = Ak[(size_t)i * Wk + c];
        r[gi] += a * x[gj]; an[gi] += std::fabs(a * x[gj]);
        if (c >= 9) { r[gj] += a * x[gi]; an[gj] += std::fabs(a * x[gi]); }  // the mirror image below the diagonal blocks
      }
  }
  double worst = 0.0;
  if (map_ptr) {
    for (int j = 0; j < n_free; ++j) {
      double res = 0.0, scale = 0.0;
      for (int q = map_ptr[j]; q < map_ptr[j + 1]; ++q) {
        const size_t g = (size_t)map_mem[q];
        res += Ab[nA + g] - r[g];
        scale += an[g] + std::fabs(Ab[nA + g]);
      }
      worst = std::max(worst, scale > 0.0 ? std::fabs(res) / scale : 0.0);
    }
  } else
  for (size_t g = 0; g < n9; ++g)
    if (!is_gauge_slot((long long)g, axis)) {
      const double bg = Ab[nA + g], scale = an[g] + std::fabs(bg);
      worst = std::max(worst, scale > 0.0 ? std::fabs(bg - r[g]) / scale : 0.0);
    }
  return worst;
}

// ------------------------------------------------------------------ what mvba_debug_read expands on the host
// the packed strips `pk` to the dense 9 m x 9 m matrix `out`, both triangles
inline void expand_packed_A(const double *pk, int m, double *out) {
  const size_t n9 = 9 * (size_t)m;
  for (size_t r = 0; r < n9; ++r)
    for (size_t cc = 0; cc < n9; ++cc) {
      const size_t lo = std::min(r, cc), hi = std::max(r, cc);
      const int k = (int)(lo / 9), l = (int)(hi / 9);
      // inside a diagonal block both halves are stored: keep the entry as computed
      const size_t rr = (k == l) ? r : lo, c2 = (k == l) ? cc : hi;
      out[r * n9 + cc] = pk[strip_offset(k, m) + (rr - 9 * k) * (size_t)(9 * (m - k)) + (c2 - 9 * k)];
    }
}

// The full 128-byte record of an observation (16 doubles: slot s = (row 0, row 1) at [2 s], [2 s + 1]; J_X 0..2, d/df 3, J_omega 4..6,
// residual 7) from the compact one (`c8`: slots 0..3), its residual, its point and its camera's centre, as mvba_debug_read hands
// it out: J_omega = (row of J_X) x (X - t), the expression of obs_math and of k_schur_lanes_compact.
inline void expand_compact_record(const double *c8, const double *e2, const double *X3, const double *t3, double *full16) {
  for (int i = 0; i < 8; ++i) full16[i] = c8[i];
  const double d[3] = {X3[0] - t3[0], X3[1] - t3[1], X3[2] - t3[2]};
  for (int i = 0; i < 3; ++i) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    for (int rr = 0; rr < 2; ++rr) full16[8 + 2 * i + rr] = c8[2 * i1 + rr] * d[i2] - c8[2 * i2 + rr] * d[i1];
  }
  full16[14] = e2[0];
  full16[15] = e2[1];
}
// A full record `q16` as the C interface's rows: the residual [2], J_X [2][3], J_C [2][9] = d/df | (u, v) | -J_X | J_omega.  The
// (u, v) columns are implied: cu = 1 / f0, or sqrt(w) / f0 under a robust loss, as the Schur kernels take them.
inline void record_to_residual(const double *q16, double *out2) { out2[0] = q16[14]; out2[1] = q16[15]; }
inline void record_to_JX(const double *q16, double *out6) {
  for (int rr = 0; rr < 2; ++rr) for (int i = 0; i < 3; ++i) out6[3 * rr + i] = q16[2 * i + rr];
}
inline void record_to_JC(const double *q16, double cu, double *out18) {
  for (int rr = 0; rr < 2; ++rr) {
    out18[9 * rr + 0] = q16[6 + rr];
    out18[9 * rr + 1] = rr == 0 ? cu : 0.0;
    out18[9 * rr + 2] = rr == 1 ? cu : 0.0;
    for (int i = 0; i < 3; ++i) out18[9 * rr + 3 + i] = -q16[2 * i + rr];
    for (int i = 0; i < 3; ++i) out18[9 * rr + 6 + i] = q16[8 + 2 * i + rr];
  }
}

// ------------------------------------------------------------------ cam15, the engine's camera row
// f | u (2) | t (3) | R (9, row-major) -- to and from the C interface's arrays
inline void pack_cam15(int m, const double *f, const double *u, const double *t, const double *R, double *cam /*[m][CAM_IN]*/) {
  for (int k = 0; k < m; ++k) {
    double *c = cam + (size_t)k * CAM_IN;
    c[0] = f[k]; c[1] = u[2 * k]; c[2] = u[2 * k + 1];
    for (int i = 0; i < 3; ++i) c[3 + i] = t[3 * k + i];
    for (int i = 0; i < 9; ++i) c[6 + i] = R[9 * k + i];
  }
}
inline void unpack_cam15(const double *cam /*[m][CAM_IN]*/, int m, double *f, double *u, double *t, double *R) {
  for (int k = 0; k < m; ++k) {
    const double *c = cam + (size_t)k * CAM_IN;
    f[k] = c[0]; u[2 * k] = c[1]; u[2 * k + 1] = c[2];
    for (int i = 0; i < 3; ++i) t[3 * k + i] = c[3 + i];
    for (int i = 0; i < 9; ++i) R[9 * k + i] = c[6 + i];
  }
}

// ------------------------------------------------------------------ the lane form's index row and its point ranges
// An item of a 64-wide step (k_schur_lanes, mvba_lanes.h) is TWO words: the k-side record, the point row and the l-side record as
// its offset from k -- k and l are observations of one point, l >= k, so l - k is below that point's degree.  Records are indexed
// from their range's first observation and gathered with 32-bit byte offsets of 128-byte rows, point rows likewise from the
// array's start (the padding row is row N): both are below 2^25 by the guards decide_schur_form has for those offsets.  That
// leaves 2 x 7 bits for the offset:
//   w0 = k | (l - k)[0..6] << 25        w1 = a | (l - k)[7..13] << 25
// A padding item is (0, 0, N), a diagonal item has l = k.
constexpr int LANE_IDX_ROW_BITS = 25, LANE_IDX_OFF_BITS = 2 * (32 - LANE_IDX_ROW_BITS);
constexpr unsigned LANE_IDX_ROW_MASK = (1u << LANE_IDX_ROW_BITS) - 1, LANE_IDX_OFF_LOW = (1u << (32 - LANE_IDX_ROW_BITS)) - 1;
constexpr long long LANE_IDX_MAX_ROW = LANE_IDX_ROW_MASK, LANE_IDX_MAX_OFF = (1LL << LANE_IDX_OFF_BITS) - 1;
struct LaneIdx { unsigned w0, w1; };
__host__ __device__ constexpr LaneIdx lane_idx_pack(int k, int l, int a) {
  const unsigned d = (unsigned)(l - k);
  return {(unsigned)k | (d & LANE_IDX_OFF_LOW) << LANE_IDX_ROW_BITS, (unsigned)a | (d >> (32 - LANE_IDX_ROW_BITS)) << LANE_IDX_ROW_BITS};
}
// (the kernel's gather lanes each need one of the three, of another item: the fields one by one)
__host__ __device__ constexpr int lane_idx_k(unsigned w0) { return (int)(w0 & LANE_IDX_ROW_MASK); }
__host__ __device__ constexpr int lane_idx_a(unsigned w1) { return (int)(w1 & LANE_IDX_ROW_MASK); }
__host__ __device__ constexpr int lane_idx_l(unsigned w0, unsigned w1) {
  return (int)((w0 & LANE_IDX_ROW_MASK) + (w0 >> LANE_IDX_ROW_BITS) + ((w1 >> LANE_IDX_ROW_BITS) << (32 - LANE_IDX_ROW_BITS)));
}
__host__ __device__ constexpr void lane_idx_unpack(LaneIdx p, int &k, int &l, int &a) {
  k = lane_idx_k(p.w0); l = lane_idx_l(p.w0, p.w1); a = lane_idx_a(p.w1);
}
// What a scene must keep to for the packed row: N points (row N is the padding row), the longest range of `widest` observations,
// the largest degree of a point.  The first two restate the byte-offset guards; the third is the packed row's own.
constexpr bool lane_idx_fits(long long N, long long widest, long long max_degree) {
  return N <= LANE_IDX_MAX_ROW && widest - 1 <= LANE_IDX_MAX_ROW && max_degree - 1 <= LANE_IDX_MAX_OFF;
}
static_assert((1LL << 32) / 128 - 2 <= LANE_IDX_MAX_ROW, "the largest N (and range) with (N + 1) * 128 < 2^32 fits the row fields");

// Point ranges of the lane form.  Its launch is not paced and its waves need not be resident together, so the ranges are
// counted by the chip's wave places (CUs x waves of the kernel per CU, from the occupancy query), not by XCDs: the largest nR
// with nR x range_waves <= places, so that every wave starts at once and the lists are as short as that allows.  Capped as the
// slot form caps its own (8 x (1 .. 8), while the typical list keeps 64 items per range); at least 1.  `forced` > 0
// (MVBA_SLOT_RANGES) is taken as it is, up to the cap's ceiling: more waves than places only run later.
constexpr int LANE_MAX_RANGES = 64;
inline int lane_ranges(long long places, long long range_waves, long long target, int forced) {
  if (forced > 0) return std::min(forced, LANE_MAX_RANGES);
  const long long cap = 8 * std::max<long long>(1, std::min<long long>(LANE_MAX_RANGES / 8, target / (8 * 64)));
  return (int)std::max<long long>(1, std::min(places / std::max<long long>(1, range_waves), cap));
}

// Which wave b = nR w + r (wave w of range r, the numbering of the index) block B of the lane form's launch is.  Blocks go to the
// XCDs round-robin, B % 8.  A range whose waves share an XCD reads its records through ONE L2; striped over all eight, ten
// ranges ran 18 % SLOWER than eight.  So with nR = 8 q + s the ranges x, x + 8, .. of the first 8 q are XCD x's
// own, wave-major, and the waves of the s surplus ranges are dealt over the XCDs behind them.  For s = 0 and for nR < 8 this is
// b = B.  `range_waves` = waves per range (blocks / nR).
__host__ __device__ constexpr int lane_wave_of_block(int B, int nR, int range_waves) {
  const int q = nR / 8, s = nR - 8 * q, i = B / 8, x = B % 8, home = q * range_waves;
  if (i < home) return nR * (i / q) + x + 8 * (i % q);
  const int j = 8 * (i - home) + x;
  return nR * (j / s) + 8 * q + j % s;
}

// ------------------------------------------------------------------ width rules: the value a launch takes, the domain beside it
// K5: lanes per point by mean degree
constexpr int K5_LANES[] = {2, 4, 8};
inline int k5_lanes(double mean_degree) { return mean_degree <= 40.0 ? 2 : (mean_degree <= 100.0 ? 4 : 8); }
// Threads of a block that holds a camera table of `lds_bytes` in LDS.  16 waves per CU is what the registers allow: 256-thread
// blocks reach it while four of them fit -- tables up to 40 KiB, ~180 cameras of K5 --, 512-thread blocks while two fit, one
// 1024-thread block beyond (a table above half the LDS leaves one block per CU).  The cost pass stops at 512.
constexpr int TABLE_BLOCK_THREADS[] = {256, 512, 1024};
inline int table_block_threads(size_t lds_bytes) { return lds_bytes > 80 * 1024 ? 1024 : (lds_bytes > 40 * 1024 ? 512 : 256); }
// the covariance's point pass: lanes per point by mean pair count, d (d + 1) / 2 at mean degree d
constexpr int COV_LANES[] = {8, 16, 32, 64};
inline int cov_lanes(double mean_pairs) { return mean_pairs > 48.0 ? 64 : (mean_pairs > 24.0 ? 32 : (mean_pairs > 12.0 ? 16 : 8)); }

}  // namespace mvba
