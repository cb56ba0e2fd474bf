// K3, slot form with ONE LANE PER ITEM (k_schur_lanes: 64 lists per wave; included by mvba.hip in the middle of its K3 section,
// it uses that file's constants and shared pieces: SchurStage, lds_gather16, lds_index_row, schur_item, jc_sign).  A lane
// owns one list -- the items of one (pair, sub-list) inside one point range -- and keeps that pair's WHOLE 9 x 9 block in its
// registers (81 fp64 accumulators; the three-lanes-per-item form of k_schur_slots keeps 27 per lane and forms
// t = J_Xk E^-1 J_Xl^T three times per item).  Per item: 272 instead of ~780 bytes of LDS reads (a lane reads its own rows
// once), a third of the index rows and of the scalar bookkeeping; the row gathers (3 per item) are the same.  What it costs: a
// step stages 64 x 272 B = 17,408 B, three buffers (two gathers in flight) + a two-deep index ring are 53,760 B per wave --
// THREE waves per CU, 96 per XCD -- so every latency is hidden by the wave's own software pipeline or not at all, and a point
// range's lists must fit 96 waves (mvba_create: ~100 cameras at 10 % visibility).  The launch is not paced: 96 waves per XCD
// drift less than k_schur_slots' 284 (DESIGN.md §3.1 has both timings).
//
// Staging buffer of a step: SchurStage<64, DIAG, packed>, one row per lane = slot = item.  Every gather instruction is a full
// wave: 64 rows x 7 slots = 7 instructions per record side, 3 (5) for the point rows, 1 for the residuals; lane-slot
// e = 64 j + lane of instruction j is row e / 7 (e / 3, e / 5), slot e % 7, and lands at byte 16 e of its region -- the
// row-major layout.
// Index row of a step: k[64] | l[64] | a[64] (768 B, one 48-lane LDS-DMA), two deep.
// What the counted wait covers: iteration s sends the index row of step s + 3 into the ring slot whose indices (step s + 1)
// were read an iteration ago, reads the indices of step s + 2 from the OTHER slot, sends the G gathers of step s + 2 (13 DIAG,
// 17 otherwise; all unconditional, steps past the end clamped to the last one) and computes step s.  vmcnt retires in issue
// order, so "all but the last iteration's G gathers" at the top of iteration s = the gathers of step s have landed and so has
// the index row of step s + 2.
#pragma once

constexpr int LANES_W = 64;                   // slots (= lanes = items) per step
constexpr int LANES_IDX = 3 * LANES_W;        // ints per index row
constexpr int LANES_BUF = SchurStage<LANES_W, false, true>::SIZE;  // one staging buffer (the off-diagonal step is the larger one)
constexpr int LANES_LDS = 3 * LANES_BUF + 2 * LANES_IDX * 4;  // three staging buffers + the index ring per wave
static_assert(LANES_BUF == 17408 && LANES_LDS == 53760, "the launch's LDS bytes");
static_assert(SchurStage<LANES_W, true, true>::SIZE <= LANES_BUF, "a diagonal step fits the buffer");
static_assert(3 * ((LANES_LDS + 511) / 512 * 512) <= 160 * 1024, "three waves per CU");

// prologue: one index row, the gathers of steps 0 and 1 | loop: wait / issue / compute / rotate | epilogue: drain, one
// partial per lane
template <bool DIAG>
__device__ __forceinline__ void schur_lanes_run(char *wbuf, const int lane, const long long beg, const int nst,
                                                const int *__restrict__ it_x, const double2 *__restrict__ rec,
                                                const double *__restrict__ PB, const double c, const double cu,
                                                double *__restrict__ out, const int *__restrict__ slot_unit) {
  using S = SchurStage<LANES_W, DIAG, true>;
  constexpr int NPS = S::NPS, BUFSZ = S::SIZE, NBUF = 3;
  constexpr int G = DIAG ? 7 + 1 + 5 : 7 + 7 + 3;          // gathers per step
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
  const int *xring = reinterpret_cast<const int *>(wbuf + NBUF * BUFSZ);
  const int *xbase = it_x + beg * LANES_IDX;               // (`beg` = first STEP of this wave; wave-uniform)
  const int last_st = nst - 1;
  // this lane's (row, slot) of gather instruction j: records 7 slots per row, point rows NPS
  auto rec_row = [&](int j) { return (64 * j + lane) / 7; };
  auto rec_s16 = [&](int j) { return (unsigned)((64 * j + lane) % 7) << 4; };
  auto pb_row = [&](int j) { return (64 * j + lane) / NPS; };
  auto pb_s16 = [&](int j) { return (unsigned)((64 * j + lane) % NPS) << 4; };
  const unsigned lane16 = (unsigned)min(lane, 47) << 4;
  auto index_row = [&](int st, unsigned ring_off) {  // the 768-byte index row of step st -> ring slot at byte offset ring_off
    const int *src = xbase + (size_t)min(st, last_st) * LANES_IDX;  // wave-uniform
    const unsigned dst = ldsx0 + ring_off;
    if (lane < 48) lds_index_row(lane16, src, dst);
  };
  constexpr unsigned RING_B = LANES_IDX * 4;
  // one iteration's vector-memory operations: the index row of step `st_idx` into ring slot `ring_next` (its old indices were read
  // an iteration ago and consumed by that iteration's gathers), then the gathers of the step whose indices stand in ring slot
  // `ring_off` (landed: the caller's wait saw to it)
  auto issue_step = [&](unsigned ring_off, unsigned ring_next, unsigned buf_off, int st_idx) {
    index_row(st_idx, ring_next);
    const int *x = reinterpret_cast<const int *>(reinterpret_cast<const char *>(xring) + ring_off);
    const unsigned buf = lds0 + buf_off;
    int kx[7], ax[NPS], lx[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) kx[j] = x[rec_row(j)];
#pragma unroll
    for (int j = 0; j < NPS; ++j) ax[j] = x[2 * LANES_W + pb_row(j)];
#pragma unroll
    for (int j = 0; j < 7; ++j) lx[j] = DIAG ? (j == 0 ? x[lane] : 0) : x[LANES_W + rec_row(j)];
#pragma unroll
    for (int j = 0; j < 7; ++j) asm volatile("" : "+v"(kx[j]), "+v"(lx[j]));  // (the reads are issued here, ahead of the gathers)
#pragma unroll
    for (int j = 0; j < NPS; ++j) asm volatile("" : "+v"(ax[j]));
    if (!DIAG) {
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

  // the arithmetic of one step on a landed buffer: this lane's item
  auto compute = [&](const char *buf) {
    const double2 *kr = reinterpret_cast<const double2 *>(buf + lane * PROW);
    const double2 *lr = DIAG ? kr : reinterpret_cast<const double2 *>(buf + S::L + lane * PROW);
    const double *pb = reinterpret_cast<const double *>(buf + S::P + lane * (16 * NPS));
    const double2 kx0 = kr[0], kx1 = kr[1], kx2 = kr[2];
    const double2 lx0 = lr[0], lx1 = lr[1], lx2 = lr[2];
    double t00, t01, t10, t11, w0, w1, wgt;
    schur_item<DIAG, true>(kx0, kx1, kx2, lx0, lx1, lx2, pb, buf, S::L, lane, t00, t01, t10, t11, w0, w1, wgt);
    // the nine columns of J_Cl (f | u, v | t | omega; signs and 1 / f0 are applied at the end): v_j = t (sx_j, sy_j)
    const double2 lf = lr[3], lw0 = lr[4], lw1 = lr[5], lw2 = lr[6];
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
    const double2 kf = kr[3];
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
    const double2 kw0 = kr[4], kw1 = kr[5], kw2 = kr[6];
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
  issue_step(0, RING_B, 0, 1);
  if (DIAG) asm volatile("s_waitcnt vmcnt(13)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(17)" ::: "memory");
  issue_step(RING_B, 0, BUFSZ, 2);
  unsigned b0 = 0, b1 = BUFSZ, b2 = 2 * BUFSZ, r0 = 0, r1 = RING_B;  // buffers of step st, st + 1, st + 2; ring slots of step st + 2, st + 3
  for (int st = 0; st < nst; ++st) {
    // step st has landed and the indices of step st + 2 are in the ring: everything but the last iteration's gathers is done
    if (DIAG) asm volatile("s_waitcnt vmcnt(13)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(17)" ::: "memory");
    issue_step(r0, r1, b2, st + 3);  // step st + 2 (past the end: the clamped last step once more, into a buffer nobody reads)
    compute(wbuf + b0);
    { const unsigned tb = b0, tr = r0; b0 = b1; b1 = b2; b2 = tb; r0 = r1; r1 = tr; }  // rotate (as in schur_slots_run; the ring is two deep)
  }
  static_assert(SLOT_OPS == (DIAG ? 13 : 17), "counted wait");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped gathers still in flight land in this wave's LDS
  const int u = slot_unit[lane];
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
