// K3, slot form with ONE LANE PER ITEM (k_schur_lanes: 64 lists per wave; included by mvba.hip in the middle of its K3 section,
// it uses that file's constants and shared pieces: SchurStage, lds_gather16, lds_index_row, schur_item, jc_sign).  A lane
// owns one list -- the items of one (pair, sub-list) inside one point range -- and keeps that pair's WHOLE 9 x 9 block in its
// registers (81 fp64 accumulators; the three-lanes-per-item form of k_schur_slots keeps 27 per lane and forms
// t = J_Xk E^-1 J_Xl^T three times per item).  Per item: 272 instead of ~780 bytes of LDS reads (a lane reads its own rows
// once), a third of the index rows and of the scalar bookkeeping; the row gathers (3 per item) are the same.  What it costs: a
// step stages 64 x 272 B = 17,408 B, three buffers (two gathers in flight) + a two-deep index ring are 53,248 B per wave --
// THREE waves per CU (the compact record below: FOUR, one per SIMD) -- so every latency is hidden by the wave's own software
// pipeline or not at all, and a point range's lists must fit 96 waves (mvba_create: ~100 cameras at 10 % visibility).  The
// launch is not paced -- 96 waves per range drift less than k_schur_slots' 284 (DESIGN.md §3.1 has both timings) -- and no wave
// waits for another: the point ranges are counted from the chip's wave places (lane_ranges), any number from 1 on, and a wave
// that finds no place only runs later.  Block -> (wave, range): lane_wave_of_block, a range on one XCD where that can be.
//
// Staging buffer of a step: SchurStage<64, DIAG, packed>, one row per lane = slot = item.  Every gather instruction is a full
// wave: 64 rows x 7 slots = 7 instructions per record side, 3 (5) for the point rows, 1 for the residuals; lane-slot
// e = 64 j + lane of instruction j is row e / 7 (e / 3, e / 5), slot e % 7, and lands at byte 16 e of its region -- the
// row-major layout.
// Index row of a step: w0[64] | w1[64], two packed words per item (lane_idx_pack in mvba_engine_host.h: k, l - k, a; 512 B, one
// 32-lane LDS-DMA), two deep.  A gather lane unpacks the one field it needs, of the item whose row it fetches.
// What the counted wait covers: iteration s sends the index row of step s + 3 into the ring slot whose indices (step s + 1)
// were read an iteration ago, reads the indices of step s + 2 from the OTHER slot, sends the G gathers of step s + 2 (13 DIAG,
// 17 otherwise; all unconditional, steps past the end clamped to the last one) and computes step s.  vmcnt retires in issue
// order, so "all but the last iteration's G gathers" at the top of iteration s = the gathers of step s have landed and so has
// the index row of step s + 2.
//
// COMPACT (k_schur_lanes_compact, the engines of the compact record: DESIGN.md §2, §3.3): a record row is slots 0..3 -- J_X and
// d/df, 64 B at a stride of 64 B in memory -- and the item's point row brings X_a along (slots 6, 7 of PB, which with 0..2 /
// 0..4 are ONE run of the 128-byte line read as a ring).  The lane keeps the centres t_k, t_l of its pair (12 VGPRs, loaded
// once) and forms the omega rows of either side as (row of J_X) x (X_a - t), obs_math's expression on the stored J_X: 15 fp64
// operations per side instead of 48 gathered bytes.  Gathers per step: 4 + 4 + 5 = 13 instead of 17 (DIAG: 4 + 1 + 7 = 12
// instead of 13; the residual comes from its own array); a step stages 64 x 208 B = 13,312 B, a wave holds 3 x 13,312 + 1,024 =
// 40,960 B -- exactly 80 LDS granules, FOUR waves in a CU's 160 KiB, which the 768-byte index rows missed by 512 B a wave.  (Four
// staging buffers at three waves -- a third step in flight, 54,272 B -- were built beside it and lost: DESIGN.md §3.3.)  64-byte rows put the 16 lanes of a ds_read_b128 group on four bank quads; slot s of row r therefore
// sits at position s ^ ((r >> 2) & 3) of its row -- the gather fetches it there -- and the reads are conflict-free again.
#pragma once

constexpr int LANES_W = 64;                   // slots (= lanes = items) per step
constexpr int LANES_IDX = 2 * LANES_W;        // ints per index row: w0[64] | w1[64] (lane_idx_pack, mvba_engine_host.h)
constexpr int LANES_BUF = SchurStage<LANES_W, false, true>::SIZE;  // one staging buffer (the off-diagonal step is the larger one)
constexpr int LANES_LDS = 3 * LANES_BUF + 2 * LANES_IDX * 4;  // three staging buffers + the index ring per wave
static_assert(LANES_BUF == 17408 && LANES_LDS == 53248, "the launch's LDS bytes");
static_assert(SchurStage<LANES_W, true, true>::SIZE <= LANES_BUF, "a diagonal step fits the buffer");
static_assert(3 * ((LANES_LDS + 511) / 512 * 512) <= 160 * 1024 && 4 * ((LANES_LDS + 511) / 512 * 512) > 160 * 1024, "three waves per CU");
constexpr int LANES_BUF_C = SchurStage<LANES_W, false, true, true>::SIZE;  // the same on the compact record
constexpr int LANES_LDS_C = 3 * LANES_BUF_C + 2 * LANES_IDX * 4;
static_assert(LANES_BUF_C == 13312 && LANES_LDS_C == 40960, "the compact launch's LDS bytes");
static_assert(SchurStage<LANES_W, true, true, true>::SIZE == 12288, "a compact diagonal step fits the buffer");
static_assert(4 * ((LANES_LDS_C + 511) / 512 * 512) <= 160 * 1024 && 5 * ((LANES_LDS_C + 511) / 512 * 512) > 160 * 1024, "four waves per CU, one per SIMD");

// what the compact form takes beside the records: the residuals (of the wave's range, like `rec`), the units (w = k << 16 | l)
// and the committed cameras, for the centres
struct LanesCompact {
  const double2 *res = nullptr;
  const int4 *units = nullptr;
  const double *cam15 = nullptr;
};
// lds_gather16 for rows of 1 << SH bytes (the compact records: 64, the residuals: 16)
template <int SH>
__device__ __forceinline__ void lds_gather16_rows(int row, unsigned slot16, const void *base, unsigned lds) {
  unsigned o;
  asm volatile("s_mov_b32 m0, %4\n\tv_lshl_add_u32 %0, %1, %5, %2\n\tglobal_load_lds_dwordx4 %0, %3" : "=&v"(o) : "v"(row), "v"(slot16), "s"(base), "s"(lds), "i"(SH) : "memory");
}
// the counted wait of a loop with G gathers per step
template <int G>
__device__ __forceinline__ void lanes_wait() {
  static_assert(G == 12 || G == 13 || G == 17, "the loops of k_schur_lanes and k_schur_lanes_compact");
  if (G == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if (G == 13) asm volatile("s_waitcnt vmcnt(13)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(17)" ::: "memory");
}

// prologue: one index row, the gathers of steps 0 and 1 | loop: wait / issue / compute / rotate | epilogue: drain, one
// partial per lane
template <bool DIAG, bool COMPACT = false>
__device__ __forceinline__ void schur_lanes_run(char *wbuf, const int lane, const long long beg, const int nst,
                                                const int *__restrict__ it_x, const double2 *__restrict__ rec,
                                                const double *__restrict__ PB, const double c, const double cu,
                                                double *__restrict__ out, const int *__restrict__ slot_unit, const LanesCompact cx = {}) {
  using S = SchurStage<LANES_W, DIAG, true, COMPACT>;
  constexpr int NPS = S::NPS, BUFSZ = S::SIZE, NBUF = 3;
  constexpr int RSL = COMPACT ? 4 : 7;                      // record slots staged per side
  constexpr int G = DIAG ? RSL + 1 + NPS : RSL + RSL + NPS;  // gathers per step
  double acc[9][9];
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[i][j] = 0.0;
  double dg[9], rb[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) dg[j] = rb[j] = 0.0;

  const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) char *)wbuf;
  const unsigned ldsx0 = lds0 + NBUF * BUFSZ;              // the index ring (two rows)
  const unsigned *xring = reinterpret_cast<const unsigned *>(wbuf + NBUF * BUFSZ);
  const int *xbase = it_x + beg * LANES_IDX;               // (`beg` = first STEP of this wave; wave-uniform)
  const int last_st = nst - 1;
  // this lane's (row, slot) of gather instruction j: records 7 slots per row, point rows NPS; COMPACT: records 4 slots per row,
  // fetched into their swizzled position, point rows from slot 6 on round the line
  auto rec_row = [&](int j) { return (64 * j + lane) / RSL; };
  auto rec_s16 = [&](int j) { return COMPACT ? (unsigned)((lane & 3) ^ ((lane >> 4) & 3)) << 4 : (unsigned)((64 * j + lane) % 7) << 4; };
  auto pb_row = [&](int j) { return (64 * j + lane) / NPS; };
  auto pb_s16 = [&](int j) { return (unsigned)(COMPACT ? ((64 * j + lane) % NPS + 6) & 7 : (64 * j + lane) % NPS) << 4; };
  const unsigned lane16 = (unsigned)min(lane, 31) << 4;
  auto index_row = [&](int st, unsigned ring_off) {  // the 512-byte index row of step st -> ring slot at byte offset ring_off
    const int *src = xbase + (size_t)min(st, last_st) * LANES_IDX;  // wave-uniform
    const unsigned dst = ldsx0 + ring_off;
    if (lane < 32) lds_index_row(lane16, src, dst);
  };
  constexpr unsigned RING_B = LANES_IDX * 4;
  // one iteration's vector-memory operations: the index row of step `st_idx` into ring slot `ring_next` (its old indices were read
  // an iteration ago and consumed by that iteration's gathers), then the gathers of the step whose indices stand in ring slot
  // `ring_off` (landed: the caller's wait saw to it)
  auto issue_step = [&](unsigned ring_off, unsigned ring_next, unsigned buf_off, int st_idx) {
    index_row(st_idx, ring_next);
    const unsigned *x = reinterpret_cast<const unsigned *>(reinterpret_cast<const char *>(xring) + ring_off);
    const unsigned buf = lds0 + buf_off;
    // the words of the items this lane gathers for: w0 of its record rows' items, w1 of its point rows' items and -- for the l
    // side, k + offset -- w1 of the record rows' items too (DIAG: l = k, the residual row is this lane's own item's)
    unsigned k0[RSL], a1[NPS], l1[RSL];
#pragma unroll
    for (int j = 0; j < RSL; ++j) k0[j] = x[rec_row(j)];
#pragma unroll
    for (int j = 0; j < NPS; ++j) a1[j] = x[LANES_W + pb_row(j)];
#pragma unroll
    for (int j = 0; j < RSL; ++j) l1[j] = DIAG ? (j == 0 ? x[lane] : 0u) : x[LANES_W + rec_row(j)];
#pragma unroll
    for (int j = 0; j < RSL; ++j) asm volatile("" : "+v"(k0[j]), "+v"(l1[j]));  // (the reads are issued here, ahead of the gathers)
#pragma unroll
    for (int j = 0; j < NPS; ++j) asm volatile("" : "+v"(a1[j]));
    int kx[RSL], ax[NPS], lx[RSL];
#pragma unroll
    for (int j = 0; j < RSL; ++j) {
      kx[j] = lane_idx_k(k0[j]);
      lx[j] = DIAG ? (j == 0 ? lane_idx_k(l1[0]) : 0) : lane_idx_l(k0[j], l1[j]);
    }
#pragma unroll
    for (int j = 0; j < NPS; ++j) ax[j] = lane_idx_a(a1[j]);
    if constexpr (COMPACT) {
#pragma unroll
      for (int j = 0; j < RSL; ++j) {
        lds_gather16_rows<6>(kx[j], rec_s16(j), rec, buf + 1024 * j);
        if (!DIAG) lds_gather16_rows<6>(lx[j], rec_s16(j), rec, buf + S::L + 1024 * j);
      }
      if (DIAG) lds_gather16_rows<4>(lx[0], 0u, cx.res, buf + S::L);  // l-side == k-side: only the residual is fetched
    } else if (!DIAG) {
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        lds_gather16(kx[j], rec_s16(j), rec, buf + 1024 * j);
        lds_gather16(lx[j], rec_s16(j), rec, buf + S::L + 1024 * j);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 7; ++j) lds_gather16(kx[j], rec_s16(j), rec, buf + 1024 * j);
      lds_gather16(lx[0], 7u << 4, rec, buf + S::L);  // l-side == k-side: only the residual (slot 7) is fetched
    }
#pragma unroll
    for (int j = 0; j < NPS; ++j) lds_gather16(ax[j], pb_s16(j), PB, buf + S::P + 1024 * j);
  };

  // COMPACT: the centres of this lane's pair (a lane without a list gathers padding rows only: J_X = 0, any finite centre does)
  int unit = -1;
  double tk[3] = {0.0, 0.0, 0.0}, tl[3] = {0.0, 0.0, 0.0};
  if constexpr (COMPACT) {
    unit = slot_unit[lane];
    if (unit >= 0) {
      const int kl = cx.units[unit].w;
      const double *ck = cx.cam15 + (size_t)((unsigned)kl >> 16) * CAM_IN + 3, *cl = cx.cam15 + (size_t)(kl & 0xffff) * CAM_IN + 3;
#pragma unroll
      for (int i = 0; i < 3; ++i) { tk[i] = ck[i]; tl[i] = DIAG ? tk[i] : cl[i]; }
    }
  }

  // the arithmetic of one step on a landed buffer: this lane's item
  auto compute = [&](const char *buf) {
    const double2 *kr = reinterpret_cast<const double2 *>(buf + lane * S::ROW);
    const double2 *lr = DIAG ? kr : reinterpret_cast<const double2 *>(buf + S::L + lane * S::ROW);
    const double *prow = reinterpret_cast<const double *>(buf + S::P + lane * (16 * NPS));
    const double *pb = COMPACT ? prow + 4 : prow;  // (COMPACT: X_a leads the row)
    const int sw = COMPACT ? (lane >> 2) & 3 : 0;  // position of slot s in a 64-byte row: s ^ sw
    const double2 kx0 = kr[0 ^ sw], kx1 = kr[1 ^ sw], kx2 = kr[2 ^ sw];
    const double2 lx0 = lr[0 ^ sw], lx1 = lr[1 ^ sw], lx2 = lr[2 ^ sw];
    double t00, t01, t10, t11, w0, w1, wgt;
    schur_item<DIAG, true>(kx0, kx1, kx2, lx0, lx1, lx2, pb, buf, S::L, lane, t00, t01, t10, t11, w0, w1, wgt);
    // omega rows of a side from its J_X rows: (j x d)_i = j[i+1] d[i+2] - j[i+2] d[i+1] (obs_math's expression), d = X_a - t
    auto omega = [&](const double2 j0, const double2 j1, const double2 j2, const double (&t)[3], double2 &o0, double2 &o1, double2 &o2) {
      const double d0 = prow[0] - t[0], d1 = prow[1] - t[1], d2 = prow[2] - t[2];
      o0 = make_double2(j1.x * d2 - j2.x * d1, j1.y * d2 - j2.y * d1);
      o1 = make_double2(j2.x * d0 - j0.x * d2, j2.y * d0 - j0.y * d2);
      o2 = make_double2(j0.x * d1 - j1.x * d0, j0.y * d1 - j1.y * d0);
    };
    // the nine columns of J_Cl (f | u, v | t | omega; signs and 1 / f0 are applied at the end): v_j = t (sx_j, sy_j)
    const double2 lf = lr[3 ^ sw];
    double2 lw0, lw1, lw2;
    if constexpr (COMPACT) omega(lx0, lx1, lx2, tl, lw0, lw1, lw2);
    else { lw0 = lr[4]; lw1 = lr[5]; lw2 = lr[6]; }
    const double sx[9] = {lf.x, 1.0, 0.0, lx0.x, lx1.x, lx2.x, lw0.x, lw1.x, lw2.x};
    const double sy[9] = {lf.y, 0.0, 1.0, lx0.y, lx1.y, lx2.y, lw0.y, lw1.y, lw2.y};
    double v0[9], v1[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      if (j == 1) { v0[j] = t00; v1[j] = t10; }
      else if (j == 2) { v0[j] = t01; v1[j] = t11; }
      else { v0[j] = t00 * sx[j] + t01 * sy[j]; v1[j] = t10 * sx[j] + t11 * sy[j]; }
      if (DIAG) {
        dg[j] = fma(wgt, sx[j] * sx[j] + sy[j] * sy[j], dg[j]);
        rb[j] += sx[j] * w0 + sy[j] * w1;
      }
    }
    const double2 kf = kr[3 ^ sw];
    // rows of J_Ck: f | u, v | t | omega; two chained FMAs into the accumulator per entry
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      acc[0][j] = fma(kf.y, v1[j], fma(kf.x, v0[j], acc[0][j]));
      acc[1][j] += v0[j];
      acc[2][j] += v1[j];
      acc[3][j] = fma(kx0.y, v1[j], fma(kx0.x, v0[j], acc[3][j]));
      acc[4][j] = fma(kx1.y, v1[j], fma(kx1.x, v0[j], acc[4][j]));
      acc[5][j] = fma(kx2.y, v1[j], fma(kx2.x, v0[j], acc[5][j]));
    }
    double2 kw0, kw1, kw2;
    if constexpr (COMPACT) {
      if (DIAG) { kw0 = lw0; kw1 = lw1; kw2 = lw2; }
      else omega(kx0, kx1, kx2, tk, kw0, kw1, kw2);
    } else { kw0 = kr[4]; kw1 = kr[5]; kw2 = kr[6]; }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      acc[6][j] = fma(kw0.y, v1[j], fma(kw0.x, v0[j], acc[6][j]));
      acc[7][j] = fma(kw1.y, v1[j], fma(kw1.x, v0[j], acc[7][j]));
      acc[8][j] = fma(kw2.y, v1[j], fma(kw2.x, v0[j], acc[8][j]));
    }
    lds_reads_done();
  };

  // prologue = the iterations s = -2, -1 without a step to compute
  constexpr int SLOT_OPS = G;  // what stays in flight over the counted wait: the last iteration's gathers, issued behind its index row
  index_row(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (COMPACT) {  // (the centres are in their registers before the first counted wait: the loop holds no load of the compiler's)
#pragma unroll
    for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(tk[i]), "+v"(tl[i]));
  }
  issue_step(0, RING_B, 0, 1);
  lanes_wait<G>();
  issue_step(RING_B, 0, BUFSZ, 2);
  unsigned b0 = 0, b1 = BUFSZ, b2 = 2 * BUFSZ, r0 = 0, r1 = RING_B;  // buffers of step st, st + 1, st + 2; ring slots of step st + 2, st + 3
  for (int st = 0; st < nst; ++st) {
    // step st has landed and the indices of step st + 2 are in the ring: everything but the last iteration's gathers is done
    lanes_wait<G>();
    issue_step(r0, r1, b2, st + 3);  // step st + 2 (past the end: the clamped last step once more, into a buffer nobody reads)
    compute(wbuf + b0);
    { const unsigned tb = b0, tr = r0; b0 = b1; b1 = b2; b2 = tb; r0 = r1; r1 = tr; }  // rotate (as in schur_slots_run; the ring is two deep)
  }
  static_assert(SLOT_OPS == (COMPACT ? (DIAG ? 12 : 13) : (DIAG ? 13 : 17)), "counted wait");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped gathers still in flight land in this wave's LDS
  const int u = COMPACT ? unit : slot_unit[lane];
  if (u >= 0) {
    double *o = out + (size_t)u * UNIT_STRIDE;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const double rs = jc_sign(i, cu);
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const double cs = jc_sign(j, cu);
        o[9 * i + j] = -4.0 * rs * cs * acc[i][j];
      }
    }
    if (DIAG) {
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const double cs = jc_sign(j, cu);
        o[81 + j] = 2.0 * c * cs * cs * dg[j];  // c * diag(G_k)   (ref :123-125)
        o[90 + j] = 2.0 * cs * rb[j];           // 2 Jc_k^T (Jx_k E^-1 dP - e)
      }
    }
  }
}
