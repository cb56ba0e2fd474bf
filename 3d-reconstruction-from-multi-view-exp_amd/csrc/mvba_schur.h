// K3, the gather forms -- kernels, gfx950: the unit form (k_schur_pairs, _big, _robust, _big_robust), the slot form with three
// lanes per item (k_schur_slots) and with one lane per item (k_schur_lanes, and k_schur_lanes_compact on the compact record; their
// step is mvba_lanes.h, included below), and k_schur_reduce, which sums the unit partials into the packed strips.
//
// Included by mvba.hip inside its device-code namespace, after mvba_linearize.h: uses REC, PBS, PACE_STRIDE, strip_offset and
// as_const / MVBA_CONST_AS of mvba_device.h.  The host launch (launch_schur) is in mvba.hip; the index these
// kernels walk is built by mvba_index.h / mvba_create.h.  Which piece lives where: DESIGN.md 3.1, "Map of K3's code".

// ------------------------------------------------------------------ K3
// Per (point a, camera k, camera l >= k) item, the 9x9 block (upper block triangle only):
//   -(F_ak^T E^-1 F_al)[i][j] = -Jc_k[:,i] . ( 2 Jx_k E^-1 ( 2 Jx_l^T Jc_l[:,j] ) )
// The diagonal item (l == k) also adds G^_k (ref :618-664 with :123-125 damping)
// and the right-hand side 2 Jc_k^T (Jx_k v_a - e_ak)   (ref :138-143, :471-517).

// ------------------------------------------------------------------ K3 (pair-major form)
// The sum above, organised by OUTPUT block instead of by camera strip (round 1).  Every (point, camera k,
// camera l >= k) triple is an "item" (built once on the host, sorted by (k, l), then by point), a
// "unit" is a contiguous run of one pair's items, and ONE WAVE owns a unit: it keeps its share of the
// 9x9 block in registers for the whole run, so there is no scatter and no atomic at all -- round 1's
// camera-strip kernel spent 75 % of its cycles in the LDS atomic pipe.  Per item the block is the
// rank-2 product  -4 Jc_k^T t Jc_l  with  t = Jx_k E^-1 Jx_l^T (2x2).
//   lanes      lane = 3 item + cg: 21 items per step, column group cg owns columns 3cg..3cg+2 of
//              the block (f,u,v | t | omega) = 27 accumulators; t is formed redundantly by the 3 lanes
//   operands   whole 128-byte lines gathered by LDS-DMA (global_load_lds_dwordx4, 8 lanes -> 7 of the
//              8 slots of a record): the k-side record, the l-side record and the point block of the
//              21 items land in wave-private LDS as 112-byte rows (28-dword stride: the 16 lanes of a
//              ds_read_b128 group hit 16 different bank quads).  Per-lane loads out of 64 different
//              lines are bound by the L1 tag rate (1 line per clock: tools/microbench/gather_lines.hip,
//              297 vs 720 lines/us/CU from L2).
//   diagonal   a (k,k) pair adds G_k (t - I/2 instead of t), the Marquardt term c * diag(G_k) and
//              the right-hand side 2 Jc_k^T (Jx_k E^-1 dP - e); its l-side DMA fetches slots 1..7 of
//              the SAME record (the residual is slot 7) and the point row is 5 slots (E^-1 dP behind
//              the inverse).  Diagonal pairs hold ~10x the items of an off-diagonal pair and are dealt
//              round-robin into sub-lists, so that all units of a strip sweep the points at one pace.
//   placement  the units of strip k run on XCD k % 8 (work queues per XCD, the wave reads its
//              XCC_ID and pulls from that queue first, then steals): the ~5.5 units that need the
//              k-side record of one observation run at the same time on the same L2.
//   output     partial[unit][104] (81 block, 9 damping, 9 rhs), summed per pair in unit order by
//              k_schur_reduce into the packed strips: bitwise reproducible, no zero-fill of A.
//
// The gather forms of K3 (DESIGN.md §3.1 has the map): the unit form above (schur_unit_run: k_schur_pairs*), the slot form
// with three lanes per item (schur_slots_run: k_schur_slots) and with one lane per item (schur_lanes_run in mvba_lanes.h:
// k_schur_lanes).  What they share comes first and is written once.
constexpr int PSTEP = 21;                       // items per wave step of the 3-lanes-per-item forms
constexpr int PROW = 7 * 16;                    // staged bytes per record (slots 0..6, or 1..7)
constexpr int UNIT_STRIDE = 104;                // doubles per unit partial
constexpr int SLOT_IDX = 64;                    // slot form: ints per step in the index (k[21] | l[21] | a[21] | pad): ONE 256-byte DMA row
constexpr int SLOT_IDX_RING = 3;                // ... staged three steps deep in LDS

// ---- the staging buffer of one step of W item rows: the ONE statement of its layout (every form takes its offsets from
// here, every launch its LDS bytes)
//   k rows [W][112 B] | l rows [W][112 B] | point rows [W][16 NPS B]      NPS = 3 slots (E^-1), DIAG: 5 (E^-1, E^-1 dP, weight)
// A diagonal step needs of its l side (the SAME record) only the residual, slot 7: [W][16 B] at the head of the l region.
// PACKED (the slot forms: three buffers in a tight LDS budget) sizes the l region and the point rows for the step at hand;
// unpacked (the unit form: a wave meets both kinds of unit) keeps the full l region and five point slots whatever the step,
// and its robust build gathers the step's sqrt(w) values (8 bytes per item: k side, then l side) at SQW, into what the
// squared build leaves unused: behind the residuals (DIAG), behind the 3-slot point rows (off-diagonal).
// COMPACT (the lane form on the compact record, mvba_lanes.h): record rows of 4 slots (J_X, d/df: 64 B) and point rows that
// carry X_a in two more slots -- 5 (X, E^-1), DIAG: 7 (X, E^-1, E^-1 dP, weight).
template <int W, bool DIAG, bool PACKED, bool COMPACT = false>
struct SchurStage {
  static_assert(!COMPACT || PACKED, "the compact rows are the slot forms'");
  static constexpr int ROW = COMPACT ? 4 * 16 : PROW;
  static constexpr int NPS = (DIAG ? 5 : 3) + (COMPACT ? 2 : 0);
  static constexpr int L = W * ROW;
  static constexpr int P = L + ((PACKED && DIAG) ? W * 16 : W * ROW);
  static constexpr int SIZE = P + W * 16 * (PACKED ? NPS : 5);
  static constexpr int SQW = DIAG ? L + W * 16 : P + W * 16 * NPS;
  static constexpr int SQW_END = SQW + (DIAG ? 1 : 2) * W * 8;
};
constexpr int PWAVE_LDS = SchurStage<PSTEP, false, false>::SIZE;  // the unit form's buffer
constexpr int SLOT_BUF = SchurStage<PSTEP, false, true>::SIZE;    // the slot form's (the off-diagonal step is the larger one)
constexpr int PAIRS_LDS = 2 * PWAVE_LDS;                          // the unit form: two staging buffers per wave
constexpr int SLOT_LDS = 3 * SLOT_BUF + SLOT_IDX_RING * SLOT_IDX * 4;  // three staging buffers + the index ring per wave: nine waves per CU
static_assert(PWAVE_LDS == 6384 && SLOT_BUF == 5712 && SLOT_LDS == 17904, "the launches' LDS bytes");
static_assert(SchurStage<PSTEP, true, false>::SIZE == PWAVE_LDS && SchurStage<PSTEP, true, true>::SIZE <= SLOT_BUF, "a diagonal step fits the buffer");
static_assert(SchurStage<PSTEP, true, false>::SQW_END <= SchurStage<PSTEP, true, false>::P && SchurStage<PSTEP, false, false>::SQW_END <= PWAVE_LDS,
              "robust weights fit the staging buffer");
// (LDS is handed out in 512-byte granules: 9 x 17,920 = 161,280 of the 163,840 bytes.  16 bytes are all a wave could still have --
// with 48 more, a CU holds eight waves, the range's 284 are no longer all resident and the launch spends 6 ms in pacing time-outs:
// profiles/r05_pace_poll.txt)
static_assert(9 * ((SLOT_LDS + 511) / 512 * 512) <= 160 * 1024, "nine waves per CU");

// ---- LDS-DMA.  lds_dma16: the compiler's builtin, for the unit form, whose waits the compiler counts.
__device__ __forceinline__ void lds_dma16(const void *gsrc, void *lds_wave_uniform) {
  __builtin_amdgcn_global_load_lds(gsrc, (__attribute__((address_space(3))) void *)lds_wave_uniform, 16, 0, 0);
}
// The slot forms keep the gathers of two steps in flight over COUNTED waits, which hipcc cannot be left to place: it drains
// the queue -- vmcnt(0) -- before any LDS read that might alias a DMA in flight.  So every vector-memory operation of their
// loops is one of the two asm statements below, which the compiler knows nothing about, and the `s_waitcnt vmcnt(N)` of the
// loops are the only waits (csrc/check_isa.py checks that on the generated code).  vmcnt retires in issue order: N = the
// operations of the last iteration, all of them unconditional (a masked-off lane still counts; a skipped instruction
// would not), none returning data to a register.
// M0 (the LDS destination base) is written in the SAME statement that uses it: it is compiler-reserved, an "m0" clobber only
// draws a warning, and the compiler's own M0 users -- none in k_schur_slots: check_isa.py fails the build if one appears --
// set it themselves.
// lds_gather16: 16 bytes per lane, base[row * 128 + slot16] -> LDS at `lds` (wave-uniform; the lanes land 16 bytes apart).
// The byte offset is formed BETWEEN the write of M0 and the gather that reads it: that is the one wait state the hardware
// asks for there.
__device__ __forceinline__ void lds_gather16(int row, unsigned slot16, const void *base, unsigned lds) {
  unsigned o;
  asm volatile("s_mov_b32 m0, %4\n\tv_lshl_add_u32 %0, %1, 7, %2\n\tglobal_load_lds_dwordx4 %0, %3" : "=&v"(o) : "v"(row), "v"(slot16), "s"(base), "s"(lds) : "memory");
}
// lds_index_row: a step's index row (at the wave-uniform `src`) -> LDS at `dst`, 16 bytes per lane at `lane16`; the caller
// masks off the lanes past the row (and clamps their lane16)
__device__ __forceinline__ void lds_index_row(unsigned lane16, const int *src, unsigned dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(lane16), "s"(src), "s"(dst) : "memory");
}
// the LDS reads of a step are complete (their values were consumed) before its buffer is refilled
__device__ __forceinline__ void lds_reads_done() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ---- J_C row (and column) i = jc_sign(i) * (record columns): f | u, v (1/f0 = cu) | t (-J_X) | omega.  The accumulators hold
// the products of the record columns; every epilogue applies the factors once, at the end.
__device__ __forceinline__ constexpr double jc_sign(int i, double cu) { return (i == 1 || i == 2) ? cu : ((i >= 3 && i < 6) ? -1.0 : 1.0); }

// ---- the arithmetic of one item: t = J_Xk E^-1 J_Xl^T (2x2) -- h = E^-1 J_Xl^T (3x2), t = J_Xk h -- and for a diagonal item
// t - I/2 (the block is then G_k) and w = J_Xk E^-1 dP - e (the right-hand side).  `pb` = the item's point row, the residual is slot
// `row` of the buffer's l region (DIAG only).  PADDED (slot forms): the point row's tenth double is 1 for a point and 0 for the padding row,
// which stands next to a real record (its range's first): the I/2 and w terms must vanish with it, like the diag(G_k) term
// in the callers.
template <bool DIAG, bool PADDED>
__device__ __forceinline__ void schur_item(const double2 kx0, const double2 kx1, const double2 kx2, const double2 lx0, const double2 lx1,
                                           const double2 lx2, const double *pb, const char *buf, const int l_off, const int row, double &t00, double &t01,
                                           double &t10, double &t11, double &w0, double &w1, double &wgt) {
  const double i00 = pb[0], i01 = pb[1], i02 = pb[2], i11 = pb[3], i12 = pb[4], i22 = pb[5];
  const double h0x = i00 * lx0.x + i01 * lx1.x + i02 * lx2.x, h0y = i00 * lx0.y + i01 * lx1.y + i02 * lx2.y;
  const double h1x = i01 * lx0.x + i11 * lx1.x + i12 * lx2.x, h1y = i01 * lx0.y + i11 * lx1.y + i12 * lx2.y;
  const double h2x = i02 * lx0.x + i12 * lx1.x + i22 * lx2.x, h2y = i02 * lx0.y + i12 * lx1.y + i22 * lx2.y;
  t00 = kx0.x * h0x + kx1.x * h1x + kx2.x * h2x, t01 = kx0.x * h0y + kx1.x * h1y + kx2.x * h2y;
  t10 = kx0.y * h0x + kx1.y * h1x + kx2.y * h2x, t11 = kx0.y * h0y + kx1.y * h1y + kx2.y * h2y;
  w0 = 0.0, w1 = 0.0;
  wgt = (DIAG && PADDED) ? pb[9] : 1.0;
  if (DIAG) {
    t00 -= PADDED ? 0.5 * wgt : 0.5;
    t11 -= PADDED ? 0.5 * wgt : 0.5;
    const double2 e = reinterpret_cast<const double2 *>(buf + l_off)[row];
    w0 = kx0.x * pb[6] + kx1.x * pb[7] + kx2.x * pb[8] - e.x;
    w1 = kx0.y * pb[6] + kx1.y * pb[7] + kx2.y * pb[8] - e.y;
    if (PADDED) {
      w0 *= wgt;
      w1 *= wgt;
    }
  }
}

// ---- the 3-lane column-group step of the 21-wide forms: lane = 3 item + cg (`it`, item row of the step), column group cg owns
// columns 3 cg .. 3 cg + 2 of the item's block (f, u, v | t | omega): 27 accumulators of the block (acc), 3 + 3 of the
// diagonal's damping (dg) and right-hand side (rb).  Column q of this lane = al12 * (l-row slot sel_q) + unit vector (bx1);
// sign and 1/f0 are applied at the end.
// One step on a landed buffer laid out as S; `ns` = its item rows.  ROBUST (unit form): the records are
// scaled by sqrt(w) already (K1), the implied (u, v) columns are not -- each item takes sqrt(w) of its k-side and l-side
// observations into its u, v rows (k side) and its u, v columns (l side)
template <class S, bool DIAG, bool PADDED, bool ROBUST>
__device__ __forceinline__ void schur_colgroup_step(const int it, const int sel0, const int sel1, const int sel2, const double al12,
                                                    const double bx1, const char *buf, const int ns,
                                                    double (&acc)[9][3], double (&dg)[3], double (&rb)[3]) {
  const char *kbuf = buf, *lbuf = buf + S::L, *pbuf = buf + S::P;
  if (it < ns) {
    double swk = 1.0, swl = 1.0;
    if (ROBUST) {
      const double *wl = reinterpret_cast<const double *>(buf + S::SQW);
      swk = wl[it];
      swl = DIAG ? swk : wl[PSTEP + it];
    }
    const double2 *kr = reinterpret_cast<const double2 *>(kbuf + it * PROW);
    const double2 *lr = DIAG ? kr : reinterpret_cast<const double2 *>(lbuf + it * PROW);
    const double *pb = reinterpret_cast<const double *>(pbuf + it * (16 * S::NPS));
    const double2 kx0 = kr[0], kx1 = kr[1], kx2 = kr[2], kf = kr[3], kw0 = kr[4], kw1 = kr[5], kw2 = kr[6];
    const double2 lx0 = lr[0], lx1 = lr[1], lx2 = lr[2];
    double t00, t01, t10, t11, w0, w1, wgt;
    schur_item<DIAG, PADDED>(kx0, kx1, kx2, lx0, lx1, lx2, pb, buf, S::L, it, t00, t01, t10, t11, w0, w1, wgt);
    const double2 s0v = lr[sel0], s1v = lr[sel1], s2v = lr[sel2];
    const double bxw = ROBUST ? bx1 * swl : bx1;  // (u, v) columns: sqrt(w) of the l-side observation
    const double sx[3] = {s0v.x, al12 * s1v.x + bxw, al12 * s2v.x};
    const double sy[3] = {s0v.y, al12 * s1v.y, al12 * s2v.y + bxw};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double v0 = t00 * sx[q] + t01 * sy[q], v1 = t10 * sx[q] + t11 * sy[q];
      // two chained FMAs into the accumulator per row (written out: `acc += a*b + c*d` compiles to
      // mul + fma + add, a third more fp64 instructions in a kernel whose VALU is 70 % busy)
      acc[0][q] = fma(kf.y, v1, fma(kf.x, v0, acc[0][q]));
      if (ROBUST) {  // (u, v) rows: sqrt(w) of the k-side observation
        acc[1][q] = fma(swk, v0, acc[1][q]);
        acc[2][q] = fma(swk, v1, acc[2][q]);
      } else {
        acc[1][q] += v0;
        acc[2][q] += v1;
      }
      acc[3][q] = fma(kx0.y, v1, fma(kx0.x, v0, acc[3][q]));
      acc[4][q] = fma(kx1.y, v1, fma(kx1.x, v0, acc[4][q]));
      acc[5][q] = fma(kx2.y, v1, fma(kx2.x, v0, acc[5][q]));
      acc[6][q] = fma(kw0.y, v1, fma(kw0.x, v0, acc[6][q]));
      acc[7][q] = fma(kw1.y, v1, fma(kw1.x, v0, acc[7][q]));
      acc[8][q] = fma(kw2.y, v1, fma(kw2.x, v0, acc[8][q]));
      if (DIAG) {
        if (PADDED) dg[q] = fma(wgt, sx[q] * sx[q] + sy[q] * sy[q], dg[q]);
        else dg[q] += sx[q] * sx[q] + sy[q] * sy[q];
        rb[q] += sx[q] * w0 + sy[q] * w1;
      }
    }
  }
  lds_reads_done();
}

// ------------------------------------------------------------------ K3, unit form: one unit (n items from `beg`) on one wave
// DIAG: the unit belongs to a (k,k) pair.  prologue: indices to registers, first gathers | loop: wait, issue the next step,
// compute this one | epilogue: the fixed-order tree over the 21 item lanes, lanes 0..2 write the partial.
// Two LDS buffers per wave: the DMA of step n+1 is issued before step n is computed, with indices
// that were loaded one step earlier still (vmcnt counts in issue order, so one wait per step covers
// both).  12 waves x 6 KB in flight per CU is what a random-line gather needs to run at the HBM
// rate (Little: 6.4 TB/s x ~2.5 us / 256 CUs).
// ROBUST: sqrt(w) per observation in `sqw`; the 21 + 21 values of a step are gathered with the step's rows (LDS-DMA, 4 bytes
// per lane, two lanes per value) to SchurStage::SQW.
template <bool DIAG, bool BIG, bool ROBUST>
__device__ __forceinline__ void schur_unit_run(char *wbuf, const int lane, const long long beg, const int n,
                                               const int *__restrict__ it_k, const int *__restrict__ it_l,
                                               const int *__restrict__ it_a, const double2 *__restrict__ rec,
                                               const double *__restrict__ PB, const double c, const double cu,
                                               double *__restrict__ out, const double *__restrict__ sqw) {
  using S = SchurStage<PSTEP, DIAG, false>;
  constexpr int NPS = S::NPS;
  const int it = lane / 3, cg = lane - 3 * it;           // compute: item of the step, column group
  const int drow = lane / 7, dslot = lane - 7 * drow;    // record DMA: 9 rows x 7 slots per instruction
  const int prow = lane / NPS, pslot = lane - NPS * prow;
  const int prow2 = (64 + lane) / 5, pslot2 = (64 + lane) - 5 * prow2;  // DIAG: second point-row DMA
  const int sel0 = cg == 0 ? 3 : (cg == 1 ? 0 : 4);
  const int sel1 = cg == 0 ? 0 : sel0 + 1, sel2 = cg == 0 ? 0 : sel0 + 2;
  const double al12 = cg == 0 ? 0.0 : 1.0, bx1 = cg == 0 ? 1.0 : 0.0;
  double acc[9][3];
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[i][q] = 0.0;
  double dg[3] = {0.0, 0.0, 0.0}, rb[3] = {0.0, 0.0, 0.0};

  // Loads and DMAs are unconditional (rows past the end of the unit are clamped to its last item and land in LDS rows
  // nobody reads): a load under a data-dependent branch makes hipcc wait vmcnt(0) per load, and so does a spilled register
  // reloaded between two DMAs -- either drains the DMAs in flight.
  int ixk[1][3], ixl[1][3], ixa[1][2];  // the next step's indices
  int ixw[2] = {0, 0};                  // ROBUST: the k-side and l-side observation of item lane / 2 of the next step
  auto load_idx = [&](int s0, int (&xk)[3], int (&xl)[3], int (&xa)[2]) {  // indices of the step starting at item s0 (to registers)
    // uniform base + unsigned 32-bit row: the saddr form again (written with int rows the clamps and the
    // address sums were done in 64 bits per lane: ~40 vector instructions per step for seven loads)
    // (the bases go through readfirstlane and the rows through an empty asm so that the compiler can neither
    // split the uniform sum into per-lane 64-bit additions nor widen the clamp to 64 bits)
    const unsigned last = (unsigned)(min(PSTEP, n - s0) - 1);
    typedef const int __attribute__((address_space(1))) *gint_p;  // (a plain pointer rebuilt from integers would be a FLAT one)
    auto uni = [](const int *p) {
      const unsigned long long v = (unsigned long long)p;
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
      return (gint_p)(((unsigned long long)hi << 32) | lo);
    };
    typedef const char __attribute__((address_space(1))) *gchar_p;
    auto row_of = [&](int r) {  // BYTE offset of the clamped row
      unsigned off = min((unsigned)r, last) << 2;
      asm("" : "+v"(off));
      return off;
    };
    auto at = [](gint_p base, unsigned off) { return *(gint_p)((gchar_p)base + off); };
    const gint_p pk = uni(it_k + (beg + s0)), pl = DIAG ? pk : uni(it_l + (beg + s0)), pa = uni(it_a + (beg + s0));
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const unsigned row = row_of(9 * q + drow);
      xk[q] = at(pk, row);
      if (!DIAG) xl[q] = at(pl, row);
    }
    if (DIAG) xl[0] = at(pk, row_of(lane));  // the record whose residual slot this lane fetches
    xa[0] = at(pa, row_of(prow));
    if (DIAG) xa[1] = at(pa, row_of(prow2));
    if (ROBUST) {
      ixw[0] = at(pk, row_of(lane >> 1));
      if (!DIAG) ixw[1] = at(pl, row_of(lane >> 1));
    }
  };
  // Addresses as "uniform base + 32-bit byte offset" (the saddr form of the memory instructions: one
  // shift-add per address instead of a sign extension, a 64-bit shift and a 64-bit add); BIG: the
  // records or the point blocks span 4 GiB or more and the offsets need 64 bits.
  auto rec_at = [&](int obs, int slot) -> const void * {
    if (BIG) return rec + (size_t)obs * REC + slot;
    return reinterpret_cast<const char *>(rec) + (((unsigned)obs << 7) + ((unsigned)slot << 4));
  };
  auto pb_at = [&](int a, int slot) -> const void * {
    if (BIG) return PB + (size_t)a * PBS + 2 * slot;
    return reinterpret_cast<const char *>(PB) + (((unsigned)a << 7) + ((unsigned)slot << 4));
  };
  auto issue = [&](char *buf, const int (&xk_)[3], const int (&xl_)[3], const int (&xa_)[2]) {
    char *kb = buf, *lb = buf + S::L, *pb_ = buf + S::P;
    const int (&xk)[3] = xk_, (&xl)[3] = xl_, (&xa)[2] = xa_;
    if (lane < 63) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        lds_dma16(rec_at(xk[q], dslot), kb + q * (9 * PROW));
        if (!DIAG) lds_dma16(rec_at(xl[q], dslot), lb + q * (9 * PROW));
      }
      if (!DIAG) lds_dma16(pb_at(xa[0], pslot), pb_);
    }
    if (lane < 7 * (PSTEP - 18)) {  // third chunk: rows 18..20 only (a buffer holds 21 rows)
      lds_dma16(rec_at(xk[2], dslot), kb + 2 * (9 * PROW));
      if (!DIAG) lds_dma16(rec_at(xl[2], dslot), lb + 2 * (9 * PROW));
    }
    if (DIAG) {  // l-side == k-side: only the residual (slot 7) is fetched, 16 bytes per item
      if (lane < PSTEP) lds_dma16(rec_at(xl[0], 7), lb);
      lds_dma16(pb_at(xa[0], pslot), pb_);
      if (lane < 5 * PSTEP - 64) lds_dma16(pb_at(xa[1], pslot2), pb_ + 1024);
    }
    if (ROBUST && lane < 2 * PSTEP) {  // sqrt(w) of the step's k-side (and l-side) observations, one dword per lane
      const char *wsrc = reinterpret_cast<const char *>(sqw) + (lane & 1) * 4;
      __builtin_amdgcn_global_load_lds(wsrc + (size_t)ixw[0] * 8, (__attribute__((address_space(3))) void *)(buf + S::SQW), 4, 0, 0);
      if (!DIAG)
        __builtin_amdgcn_global_load_lds(wsrc + (size_t)ixw[1] * 8, (__attribute__((address_space(3))) void *)(buf + S::SQW + PSTEP * 8), 4, 0, 0);
    }
  };
  auto compute = [&](const char *buf, const int ns) { schur_colgroup_step<S, DIAG, false, ROBUST>(it, sel0, sel1, sel2, al12, bx1, buf, ns, acc, dg, rb); };
  load_idx(0, ixk[0], ixl[0], ixa[0]);
  issue(wbuf, ixk[0], ixl[0], ixa[0]);
  if (PSTEP < n) load_idx(PSTEP, ixk[0], ixl[0], ixa[0]);
  for (int s0 = 0, par = 0; s0 < n; s0 += PSTEP, par ^= 1) {
    const int ns = min(PSTEP, n - s0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this step's rows have landed, the next step's indices too
    if (s0 + PSTEP < n) {
      issue(wbuf + (par ^ 1) * S::SIZE, ixk[0], ixl[0], ixa[0]);
      if (s0 + 2 * PSTEP < n) load_idx(s0 + 2 * PSTEP, ixk[0], ixl[0], ixa[0]);
    }
    compute(wbuf + par * S::SIZE, ns);
  }
  // J_C row i = rs_i * (record columns): f | u,v (1/f0) | t (-Jx) | omega; the same factors per column
  const double cs0 = cg == 1 ? -1.0 : 1.0, cs12 = cg == 0 ? cu : cs0;
  // ---- sum over the 21 item lanes of each column group (fixed tree), lanes 0..2 write the partial
  auto tree = [&](double v) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
      const double o = __shfl_down(v, 3 * off, 64);
      if (it < off && it + off < PSTEP) v += o;
    }
    return v;
  };
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double rs = jc_sign(i, cu);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double v = tree(acc[i][q]);
      if (lane < 3) out[9 * i + 3 * cg + q] = -4.0 * rs * (q == 0 ? cs0 : cs12) * v;
    }
  }
  if (DIAG) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double d = tree(dg[q]), r = tree(rb[q]);
      const double cs = q == 0 ? cs0 : cs12;
      if (lane < 3) {
        out[81 + 3 * cg + q] = 2.0 * c * cs * cs * d;  // c * diag(G_k)   (ref :123-125)
        out[90 + 3 * cg + q] = 2.0 * cs * r;           // 2 Jc_k^T (Jx_k E^-1 dP - e)
      }
    }
  }
}

// One wave per block: a wave works alone, and in a wider block its LDS and wave slots stay taken until
// the block's slowest wave has finished (4 waves per block: 1.945 ms, 2: 1.92, 1: 1.89 at config 3).
template <bool BIG, bool ROBUST>
__device__ __forceinline__ void schur_pairs_wave(const int4 *__restrict__ units, const int *__restrict__ q_ptr,
                                                       const int *__restrict__ q_units, const int *__restrict__ it_k,
                                                       const int *__restrict__ it_l, const int *__restrict__ it_a,
                                                       const double2 *__restrict__ rec,
                                                       const double *__restrict__ PB, double c, double f0,
                                                       double *__restrict__ partial, const double *__restrict__ sqw) {
  extern __shared__ char smem_pairs[];
  const int lane = threadIdx.x;
  char *wbuf = smem_pairs;
  // ---- take one unit: block b takes entry b / 8 of queue b % 8 -- no atomic on the critical path; it relies on the
  // round-robin block -> XCD placement for locality only, never for correctness (1.90 -> 1.87 ms against queues
  // taken by atomics)
  int pos = -1;
  const int x = blockIdx.x & 7, q = blockIdx.x >> 3;
  if (q < q_ptr[x + 1] - q_ptr[x]) pos = q_ptr[x] + q;
  pos = __builtin_amdgcn_readfirstlane(pos);
  if (pos < 0) return;
  // unit id (where its partial goes) and descriptor, both in queue order: two independent SCALAR loads
  // (pos is wave-uniform; read through the constant address space so that beg and n live in SGPRs and
  // the per-step index bases are scalar arithmetic)
  const int u = as_const(q_units)[pos];
  const int MVBA_CONST_AS *udp = as_const(reinterpret_cast<const int *>(units)) + 4 * (size_t)pos;
  const int ud_x = udp[0], ud_y = udp[1], ud_z = udp[2], ud_w = udp[3];
  const long long beg = ((long long)ud_y << 32) | (unsigned)ud_x;
  const int n = ud_z, cam_k = (int)((unsigned)ud_w >> 16), cam_l = ud_w & 0xffff;
  double *out = partial + (size_t)u * UNIT_STRIDE;
  if (cam_k == cam_l) schur_unit_run<true, BIG, ROBUST>(wbuf, lane, beg, n, it_k, it_l, it_a, rec, PB, c, 1.0 / f0, out, sqw);
  else schur_unit_run<false, BIG, ROBUST>(wbuf, lane, beg, n, it_k, it_l, it_a, rec, PB, c, 1.0 / f0, out, sqw);
}

#define MVBA_PAIRS_ARGS                                                                                                   \
  const int4 *__restrict__ units, const int *__restrict__ q_ptr, const int *__restrict__ q_units,                        \
      const int *__restrict__ it_k, const int *__restrict__ it_l, const int *__restrict__ it_a,                          \
      const double2 *__restrict__ rec, const double *__restrict__ PB, double c, double f0, double *__restrict__ partial
// (two plain kernels rather than one template, so that profiles show one stable name per variant)
__global__ __launch_bounds__(64, 3) void k_schur_pairs(MVBA_PAIRS_ARGS) {
  schur_pairs_wave<false, false>(units, q_ptr, q_units, it_k, it_l, it_a, rec, PB, c, f0, partial, nullptr);
}
__global__ __launch_bounds__(64, 3) void k_schur_pairs_big(MVBA_PAIRS_ARGS) {  // 64-bit record / point-block offsets
  schur_pairs_wave<true, false>(units, q_ptr, q_units, it_k, it_l, it_a, rec, PB, c, f0, partial, nullptr);
}
// robust losses: sqrt(w) per observation in `sqw`
__global__ __launch_bounds__(64, 3) void k_schur_pairs_robust(MVBA_PAIRS_ARGS, const double *__restrict__ sqw) {
  schur_pairs_wave<false, true>(units, q_ptr, q_units, it_k, it_l, it_a, rec, PB, c, f0, partial, sqw);
}
__global__ __launch_bounds__(64, 3) void k_schur_pairs_big_robust(MVBA_PAIRS_ARGS, const double *__restrict__ sqw) {
  schur_pairs_wave<true, true>(units, q_ptr, q_units, it_k, it_l, it_a, rec, PB, c, f0, partial, sqw);
}

// ------------------------------------------------------------------ K3 (slot-resident form)
// The pair-major kernel above reads every record ~5 times from beyond its L2 (89 M line misses for 10 M records at
// config 3): a unit sweeps 1/16 of the points for ONE pair, so what the ~300 units in flight on an XCD touch at
// any moment is spread over 80 MB of records.  Here the roles of the 21 item rows of a step are transposed:
//   slot     a 3-lane slot (item row `it`) owns ONE list -- the items of one (pair, sub-list) inside one point
//            range -- for the whole launch and keeps that pair's 9x9 block in its 27 registers per lane: still no
//            scatter, no atomic, no cross-lane sum at all (the fixed-order tree is gone), one partial per list
//   range    the points are cut into 8 ranges of equal item count, range r = the blocks b with b % 8 == r = XCD r
//            under the round-robin block placement (locality only, never correctness): a record is needed by ONE
//            XCD, and ALL lists of the range (m (m+1) / 2 pairs + the diagonal pairs' sub-lists: 5.9 k slots =
//            284 waves at m = 100) are resident on that XCD at once and sweep the range's points together
//   steps    built once on the host (mvba_create): the 21 lists of a wave are merged into steps with a bounded skew --
//            a slot whose next item lies more than `skew` observations ahead of the wave's slowest slot idles
//            for a step (its row points at the all-zero record / point row: the arithmetic runs and adds
//            exact zeros) -- so that what a wave touches at any moment fits its XCD's L2 next to its siblings'
// Same staging (LDS-DMA of whole lines), same arithmetic and the same partial -> k_schur_reduce path as above.

// ---- pacing of k_schur_slots: the waves of a point range keep within `lag` segments of each other, so that what they gather
// at any moment fits their XCD's L2.  `seg_end[j]` = the step at which this wave has left segment j of its point range,
// `prog[j]` = how many waves of the range have left segment j, `need` = how many there are.  A performance hint only: a wave
// that waits too long (its siblings are not resident: somebody else holds the CUs) stops pacing and runs on.  The state
// (`pacing`, `seg`, `seg_stop`) and the two places that use it (pace_at per step, the last arrivals in the epilogue) live in
// schur_slots_run: as one object with methods the loop compiled to other code (map of K3).
struct SlotPace {
  const int *seg_end;
  int *prog;
  int need, nseg, lag;
};

// ------------------------------------------------------------------ K3, slot form, three lanes per item: one wave's `nst` steps
// The 21 item rows of a step belong to 21 DIFFERENT lists: each 3-lane slot keeps its own block for the whole run and writes
// it to its own partial (`out` is the array of partials, `slot_unit` the 21 unit ids of this wave); padding rows point at
// the all-zero point row.  prologue: two index rows, the gathers of steps 0 and 1 | loop: wait / pace / issue / compute /
// rotate | epilogue: drain, the pacing's last arrivals, one partial per slot.
// Three buffers, the gathers of TWO steps in flight: a wave of this form is one serial chain of ~1400 steps
// for the whole launch and 9 of them share a CU, so what bounds it is steps-in-flight x latency, not
// throughput (per-wave stamps: 1.18 us per step with one step in flight, every wave alike).
// The step's INDEX -- 21 k-side, 21 l-side record indices and 21 points, one 256-byte row of the step-major index --
// travels through LDS too, three rows deep: ONE LDS-DMA instruction per step, read back by ordinary ds_read after the counted
// wait that covers it.
// What the counted wait covers: iteration s issues the gathers of step s + 2, then the index row of step s + 4 (into the
// ring slot whose indices, those of step s + 1, were read an iteration ago) -- 7 operations (DIAG) or 8, every one
// unconditional, steps past the end clamped to the last one.  "All but the last iteration's operations" at the top of
// iteration s = step s has landed and the indices of step s + 2 are in LDS, while step s + 1 and the indices of s + 3 stay
// in flight.
// 32-bit byte offsets only: with 64-bit per-lane addresses this loop needs more than the 168 registers of three waves per
// SIMD, and a spill's scratch access would be a vector-memory operation the counted waits do not know about.
template <bool DIAG>
__device__ __forceinline__ void schur_slots_run(char *wbuf, const int lane, const long long beg, const int nst,
                                                const int *__restrict__ it_x, const double2 *__restrict__ rec,
                                                const double *__restrict__ PB, const double c, const double cu,
                                                double *__restrict__ out, const int *__restrict__ slot_unit, const SlotPace pace) {
  using S = SchurStage<PSTEP, DIAG, true>;
  constexpr int NPS = S::NPS;
  constexpr unsigned BUFSZ = S::SIZE;
  const int it = lane / 3, cg = lane - 3 * it;           // compute: item of the step, column group
  const int drow = lane / 7, dslot = lane - 7 * drow;    // record DMA: 9 rows x 7 slots per instruction
  const int prow = lane / NPS, pslot = lane - NPS * prow;
  const int prow2 = (64 + lane) / 5, pslot2 = (64 + lane) - 5 * prow2;  // DIAG: second point-row DMA
  const int sel0 = cg == 0 ? 3 : (cg == 1 ? 0 : 4);
  const int sel1 = cg == 0 ? 0 : sel0 + 1, sel2 = cg == 0 ? 0 : sel0 + 2;
  const double al12 = cg == 0 ? 0.0 : 1.0, bx1 = cg == 0 ? 1.0 : 0.0;
  double acc[9][3];
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[i][q] = 0.0;
  double dg[3] = {0.0, 0.0, 0.0}, rb[3] = {0.0, 0.0, 0.0};

  auto compute = [&](const char *buf, const int ns) { schur_colgroup_step<S, DIAG, true, false>(it, sel0, sel1, sel2, al12, bx1, buf, ns, acc, dg, rb); };
  bool pacing = true;
  int seg = 0, seg_stop = as_const(pace.seg_end)[0] * PSTEP;
  auto pace_at = [&](const int s0) {
    while (s0 == seg_stop) {  // (wave-uniform) this wave has left segment `seg`
      if (lane == 0) __hip_atomic_fetch_add(pace.prog + PACE_STRIDE * seg, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ++seg;
      seg_stop = seg < pace.nseg ? as_const(pace.seg_end)[seg] * PSTEP : 0x7fffffff;
      if (seg >= pace.lag && pacing) {  // nobody enters segment j before everybody has left segment j - lag
        // (a waiting wave polls every ~3 us: hundreds of waves polling one word at full speed saturate the
        // fabric's atomic path and slow the arrivals they are waiting for -- 15 ms per launch, measured)
        int tries = 0;
        while (__hip_atomic_fetch_add(pace.prog + PACE_STRIDE * (seg - pace.lag), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < pace.need) {
          if (++tries > 1024) { pacing = false; break; }  // ~2 ms: the siblings are not running
          __builtin_amdgcn_s_sleep(127);
        }
        // a wave that had to wait is ahead of the pack, one that did not is among those the pack waits for: the
        // SIMD's issue arbitration (priority, then age) should favour the latter
        if (tries > 0) __builtin_amdgcn_s_setprio(0);
        else __builtin_amdgcn_s_setprio(2);
      }
    }
  };
  constexpr int SLOT_OPS = DIAG ? 7 : 8;
  const int last_st = nst - 1;
  const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) char *)wbuf;
  const unsigned ldsx0 = lds0 + 3 * SLOT_BUF;             // the index ring
  const int *xring = reinterpret_cast<const int *>(wbuf + 3 * SLOT_BUF);
  const int *xbase = it_x + beg * SLOT_IDX;               // (`beg` = first STEP of this wave; wave-uniform)
  const unsigned lane16 = (unsigned)min(lane, 15) << 4;
  auto index_row = [&](int st, unsigned ring_off) {  // the 256-byte index row of step st -> ring slot st % 3 = byte offset ring_off
    const int *src = xbase + (size_t)min(st, last_st) * SLOT_IDX;  // wave-uniform
    const unsigned dst = ldsx0 + ring_off;
    if (lane < 16) lds_index_row(lane16, src, dst);
  };
  const unsigned ds16 = (unsigned)dslot << 4, ps16 = (unsigned)pslot << 4, ps16b = (unsigned)pslot2 << 4;
  const int xr0 = min(drow, PSTEP - 1), xr1 = min(9 + drow, PSTEP - 1), xr2 = min(18 + drow, PSTEP - 1);  // this lane's rows of a step
  const int xa0 = 2 * PSTEP + min(prow, PSTEP - 1), xa1 = 2 * PSTEP + min(prow2, PSTEP - 1), xl = min(lane, PSTEP - 1);
  auto issue_step = [&](unsigned ring_off, unsigned buf_off) {  // gathers of a step from its indices in the ring (landed: the caller's wait saw to it)
    const int *x = reinterpret_cast<const int *>(reinterpret_cast<const char *>(xring) + ring_off);
    const unsigned buf = lds0 + buf_off;
    const unsigned kb = buf, lb = buf + S::L, pb_ = buf + S::P;
    const int k0 = x[xr0], k1 = x[xr1], k2 = x[xr2];
    if (!DIAG) {
      const int l0 = x[PSTEP + xr0], l1 = x[PSTEP + xr1], l2 = x[PSTEP + xr2], a0 = x[xa0];
      if (lane < 63) {
        lds_gather16(k0, ds16, rec, kb);
        lds_gather16(l0, ds16, rec, lb);
        lds_gather16(k1, ds16, rec, kb + 9 * PROW);
        lds_gather16(l1, ds16, rec, lb + 9 * PROW);
        lds_gather16(a0, ps16, PB, pb_);
      }
      if (lane < 7 * (PSTEP - 18)) {
        lds_gather16(k2, ds16, rec, kb + 18 * PROW);
        lds_gather16(l2, ds16, rec, lb + 18 * PROW);
      }
    } else {
      const int kl = x[xl], a0 = x[xa0], a1 = x[xa1];
      if (lane < 63) {
        lds_gather16(k0, ds16, rec, kb);
        lds_gather16(k1, ds16, rec, kb + 9 * PROW);
      }
      if (lane < 7 * (PSTEP - 18)) lds_gather16(k2, ds16, rec, kb + 18 * PROW);
      if (lane < PSTEP) lds_gather16(kl, 7u << 4, rec, lb);  // l-side == k-side: only the residual (slot 7) is fetched
      lds_gather16(a0, ps16, PB, pb_);
      if (lane < 5 * PSTEP - 64) lds_gather16(a1, ps16b, PB, pb_ + 1024);
    }
  };
  constexpr unsigned RING_B = SLOT_IDX * 4;
  index_row(0, 0);
  index_row(1, RING_B);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  issue_step(0, 0);
  index_row(2, 2 * RING_B);
  issue_step(last_st >= 1 ? RING_B : 0, BUFSZ);  // (a one-step wave: the clamped step 0 once more, into the buffer nobody reads)
  index_row(3, 0);
  unsigned b0 = 0, b1 = BUFSZ, b2 = 2 * BUFSZ, r0 = 0, r1 = RING_B, r2 = 2 * RING_B;  // offsets of step st, st + 1, st + 2
  for (int st = 0; st < nst; ++st) {
    // step st has landed and the indices of step st + 2 are in the ring: everything but the last iteration's operations is done
    if (DIAG) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    pace_at(st * PSTEP);
    issue_step(r2, b2);  // step st + 2 (past the end: the ring slot holds the indices of the clamped last step, its rows land in a buffer nobody reads)
    index_row(st + 4, r1);  // (st + 4) % 3 = (st + 1) % 3: the slot whose indices were read an iteration ago
    compute(wbuf + b0, PSTEP);
    // rotate: which buffer / ring slot a step uses -- step % 3 -- is carried as byte offsets (the remainders cost a dozen scalar
    // instructions a step); written out here and in schur_lanes_run: through a shared helper both loops compiled to other code
    { const unsigned tb = b0, tr = r0; b0 = b1; b1 = b2; b2 = tb; r0 = r1; r1 = r2; r2 = tr; }
  }
  static_assert(SLOT_OPS == (DIAG ? 7 : 8), "counted wait");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped gathers still in flight land in this wave's LDS
  // J_C row i = rs_i * (record columns): f | u,v (1/f0) | t (-Jx) | omega; the same factors per column
  const double cs0 = cg == 1 ? -1.0 : 1.0, cs12 = cg == 0 ? cu : cs0;
  if (lane == 0)
    for (; seg < pace.nseg; ++seg) __hip_atomic_fetch_add(pace.prog + PACE_STRIDE * seg, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int u = it < PSTEP ? slot_unit[it] : -1;
  if (u >= 0) {
    double *o = out + (size_t)u * UNIT_STRIDE;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const double rs = jc_sign(i, cu);
#pragma unroll
      for (int q = 0; q < 3; ++q) o[9 * i + 3 * cg + q] = -4.0 * rs * (q == 0 ? cs0 : cs12) * acc[i][q];
    }
    if (DIAG) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double cs = q == 0 ? cs0 : cs12;
        o[81 + 3 * cg + q] = 2.0 * c * cs * cs * dg[q];
        o[90 + 3 * cg + q] = 2.0 * cs * rb[q];
      }
    }
  }
}
__device__ __forceinline__ void schur_slots_wave(const int4 *__restrict__ wdesc, const int *__restrict__ wunits,
                                                 const int *__restrict__ it_k, const int *__restrict__ it_l,
                                                 const int *__restrict__ it_a, const double2 *__restrict__ rec,
                                                 const double *__restrict__ PB, double c, double f0,
                                                 double *__restrict__ partial, int nR, const int *__restrict__ seg_end,
                                                 int *__restrict__ prog, int nseg, int lag,
                                                 const long long *__restrict__ range_o0) {
  extern __shared__ char smem_pairs[];
  // which wave of which range: block b IS wave b / nR of range b % nR
  const int bid = blockIdx.x;
  const int MVBA_CONST_AS *dp = as_const(reinterpret_cast<const int *>(wdesc)) + 4 * (size_t)bid;
  const int d_x = dp[0], d_y = dp[1], nsteps = dp[2], flags = dp[3];
  if (nsteps <= 0) return;  // (wave-uniform) a wave whose lists are all empty in this range: no units, nothing to write
  const long long beg = ((long long)d_y << 32) | (unsigned)d_x;
  const int *su = wunits + (size_t)bid * PSTEP;
  // flags: bit 0 diagonal wave | bits 8..19 live waves of this range
  const int r = bid % nR, live = (flags >> 8) & 0xfff;
  // the record indices of the step rows are RELATIVE to the range's first observation: the 32-bit byte offsets of the
  // gathers then span a range's records (4 GiB = 33.5 M observations per range), not the scene's
  const double2 *rec_r = rec + (size_t)as_const(range_o0)[r] * REC;
  const SlotPace pace{seg_end + (size_t)bid * nseg, prog + (size_t)r * nseg * PACE_STRIDE, live, nseg, lag};
  if (flags & 1)
    schur_slots_run<true>(smem_pairs, (int)threadIdx.x, beg, nsteps, it_k, rec_r, PB, c, 1.0 / f0, partial, su, pace);
  else
    schur_slots_run<false>(smem_pairs, (int)threadIdx.x, beg, nsteps, it_k, rec_r, PB, c, 1.0 / f0, partial, su, pace);
}
#define MVBA_SLOTS_ARGS                                                                                                  \
  const int4 *__restrict__ wdesc, const int *__restrict__ wunits, const int *__restrict__ it_k, const int *__restrict__ it_l, \
      const int *__restrict__ it_a, const double2 *__restrict__ rec, const double *__restrict__ PB, double c, double f0,  \
      double *__restrict__ partial, int nR, const int *__restrict__ seg_end, int *__restrict__ prog,                      \
      int nseg, int lag, const long long *__restrict__ range_o0
__global__ __launch_bounds__(64, 3) void k_schur_slots(MVBA_SLOTS_ARGS) {
  schur_slots_wave(wdesc, wunits, it_k, it_l, it_a, rec, PB, c, f0, partial, nR, seg_end, prog, nseg, lag, range_o0);
}

#include "mvba_lanes.h"  // the slot form with one lane per item: schur_lanes_run, 64 lists per wave
constexpr int slot_idx_ints(int W) { return W == LANES_W ? LANES_IDX : SLOT_IDX; }  // ints of a step's index row at width W

// The slot form at 64 lists per wave (mvba_lanes.h): wave b = nR w + r is wave w of range r as above, its index rows are 512 bytes
// (two packed words per item) and its unit ids 64 per wave.  nR is any number from 1 on, so WHICH wave a block is keeps a range on
// one XCD where that can be (lane_wave_of_block, mvba_engine_host.h; b = blockIdx.x for a multiple of 8).  Not paced: no counters
// to clear, the pacing table of the index is not read, and no wave waits for another -- more waves than places run in turn.
__global__ __launch_bounds__(64, 1) void k_schur_lanes(const int4 *__restrict__ wdesc, const int *__restrict__ wunits,
                                                       const int *__restrict__ it_x, const double2 *__restrict__ rec,
                                                       const double *__restrict__ PB, double c, double f0,
                                                       double *__restrict__ partial, int nR,
                                                       const long long *__restrict__ range_o0) {
  extern __shared__ char smem_pairs[];
  const int bid = lane_wave_of_block((int)blockIdx.x, nR, (int)gridDim.x / nR);
  const int MVBA_CONST_AS *dp = as_const(reinterpret_cast<const int *>(wdesc)) + 4 * (size_t)bid;
  const int d_x = dp[0], d_y = dp[1], nsteps = dp[2], flags = dp[3];
  if (nsteps <= 0) return;  // (wave-uniform) a wave whose lists are all empty in this range
  const long long beg = ((long long)d_y << 32) | (unsigned)d_x;
  const int *su = wunits + (size_t)bid * LANES_W;
  const double2 *rec_r = rec + (size_t)as_const(range_o0)[bid % nR] * REC;  // record indices are relative to the range's first observation
  if (flags & 1) schur_lanes_run<true>(smem_pairs, (int)threadIdx.x, beg, nsteps, it_x, rec_r, PB, c, 1.0 / f0, partial, su);
  else schur_lanes_run<false>(smem_pairs, (int)threadIdx.x, beg, nsteps, it_x, rec_r, PB, c, 1.0 / f0, partial, su);
}
// The same on the compact record (mvba_lanes.h, COMPACT): `rec` is [n_obs + 1][REC_C], the residuals are `res` [n_obs + 1]; `units`
// (in unit order) and the committed cameras give a lane the centres of its pair.  A kernel of its own name, like the variants
// of the unit form.
__global__ __launch_bounds__(64, 1) void k_schur_lanes_compact(const int4 *__restrict__ wdesc, const int *__restrict__ wunits,
                                                               const int *__restrict__ it_x, const double2 *__restrict__ rec,
                                                               const double *__restrict__ PB, double c, double f0,
                                                               double *__restrict__ partial, int nR,
                                                               const long long *__restrict__ range_o0, const double2 *__restrict__ res,
                                                               const int4 *__restrict__ units, const double *__restrict__ cam15) {
  extern __shared__ char smem_pairs[];
  const int bid = lane_wave_of_block((int)blockIdx.x, nR, (int)gridDim.x / nR);
  const int MVBA_CONST_AS *dp = as_const(reinterpret_cast<const int *>(wdesc)) + 4 * (size_t)bid;
  const int d_x = dp[0], d_y = dp[1], nsteps = dp[2], flags = dp[3];
  if (nsteps <= 0) return;  // (wave-uniform) a wave whose lists are all empty in this range
  const long long beg = ((long long)d_y << 32) | (unsigned)d_x;
  const int *su = wunits + (size_t)bid * LANES_W;
  const long long o0 = as_const(range_o0)[bid % nR];  // record indices are relative to the range's first observation
  const LanesCompact cx{res + o0, units, cam15};
  if (flags & 1) schur_lanes_run<true, true>(smem_pairs, (int)threadIdx.x, beg, nsteps, it_x, rec + (size_t)o0 * REC_C, PB, c, 1.0 / f0, partial, su, cx);
  else schur_lanes_run<false, true>(smem_pairs, (int)threadIdx.x, beg, nsteps, it_x, rec + (size_t)o0 * REC_C, PB, c, 1.0 / f0, partial, su, cx);
}

// One thread per element of a pair's block: the pair's unit partials in unit order -> packed strips.
// One block per PAIR (blockIdx.x = packed pair index); the partials are loaded eight at a time (one
// memory latency per eight units instead of one per unit: a diagonal pair has ~130 of them) and
// added in unit order, so the result does not depend on the schedule.
__global__ __launch_bounds__(128) void k_schur_reduce(int m, const int *__restrict__ unit_ptr,
                                                      const double *__restrict__ partial, double *__restrict__ Afull,
                                                      double *__restrict__ bfull) {
  // pair index -> (k, l): pairs of strip k start at k m - k (k - 1) / 2
  const long long p = blockIdx.x;
  int k = (int)((2.0 * m + 1.0 - sqrt((2.0 * m + 1.0) * (2.0 * m + 1.0) - 8.0 * (double)p)) * 0.5);
  while ((long long)k * m - (long long)k * (k - 1) / 2 > p) --k;
  while ((long long)(k + 1) * m - (long long)(k + 1) * k / 2 <= p) ++k;
  const int l = k + (int)(p - ((long long)k * m - (long long)k * (k - 1) / 2));
  const int u0 = unit_ptr[p], u1 = unit_ptr[p + 1];
  const int e = threadIdx.x;
  if (e >= (k == l ? 99 : 81)) return;
  auto ordered_sum = [&](int off) {
    double v = 0.0;
    int uu = u0;
    for (; uu + 8 <= u1; uu += 8) {
      double t[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) t[q] = partial[(size_t)(uu + q) * UNIT_STRIDE + off];
#pragma unroll
      for (int q = 0; q < 8; ++q) v += t[q];
    }
    for (; uu < u1; ++uu) v += partial[(size_t)uu * UNIT_STRIDE + off];
    return v;
  };
  const double v = ordered_sum(e);
  double *Ak = Afull + strip_offset(k, m);
  const int Wk = 9 * (m - k);
  if (e < 81) {
    const int i = e / 9, j = e - 9 * i;
    const double d = (k == l && i == j) ? ordered_sum(81 + i) : 0.0;  // Marquardt damping of G_k's diagonal
    Ak[(size_t)i * Wk + 9 * (l - k) + j] = v + d;
  } else if (e >= 90) {
    bfull[9 * k + (e - 90)] = v;
  }
}
