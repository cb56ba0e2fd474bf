// The reduced camera system (K4) -- kernels, gfx950: gauge strip, blocked Cholesky, the two back-substitutions and the
// pivoted-LU rescue.
//
// Included by mvba.hip inside its device-code namespace, after the K3 kernels: uses strip_offset, keep_index, block_sum,
// mvba_d4, wave_sync and the status bits of mvba_common.h.  The host launches (launch_factor, launch_solve, launch_lu_solve,
// check_solve_residual) are in mvba.hip.  Which piece lives where, and which invariant it owns: DESIGN.md 3.2, "Map of K4's code".

// ------------------------------------------------------------------ K4: gauge strip + Cholesky
// The reduced system is SPD (Gauss-Newton Schur complement with Marquardt damping), so
// the reference's np.linalg.solve (LU, ref :146) is replaced by a blocked Cholesky
// (parity-safe).  Storage: M = (D+1) x ld row-major, lower triangle of A in
// rows 0..D-1 and the right-hand side b as ROW D, so that factorising carries the forward
// substitution along (row D ends up holding y = L^-1 b).  Two-level blocking: columns are
// processed in super-blocks of SBW = 128 (four 32-column panels).
//   k_chol_super  ONE launch per super-block, workgroup per 64 rows below it; every workgroup
//                 factors the 128x128 diagonal block in LDS (wave 0: tile factorisations in
//                 registers, identity rows alongside give L^-T) and solves its own rows with
//                 f64 MFMA (left-looking inside the super-block)
//   k_chol_trail64 / k_chol_trail32  once per super-block: C -= P P^T with K = 128 on v_mfma_f64_16x16x4_f64 for
//                 everything right of the super-block (64 x 64 tiles through LDS while there are >= 200 of them)
// then k_chol_backsolve_all does L^T x = y, last super-block first, from the L^-T tiles, in one persistent launch whose
// workgroups hand y to each other behind progress words.
constexpr int NB = 32;
constexpr int SBW = 4 * NB;

// Element (g1, g2) of the symmetric 9m x 9m matrix kept as packed upper strips (strip_offset)
__device__ __forceinline__ double packed_sym(const double *__restrict__ A, int m, int g1, int g2) {
  const int r = min(g1, g2), c = max(g1, g2), k = r / 9;
  return A[strip_offset(k, m) + (size_t)(r - 9 * k) * (9 * (m - k)) + (c - 9 * k)];
}

// One workgroup per 32 x 32 tile of the lower triangle (+ one per 256 columns of the right-hand-side row).  M[i][j], j <= i, is the
// packed upper element (row gj, column gi): read along gi -- the packed rows are contiguous -- and written along j, through a
// transposing LDS tile (read along gj it is one line per element).
__global__ __launch_bounds__(256) void k_compact(int D, int ld, int m, int gauge_axis, int nt, const double *__restrict__ Afull,
                                                 const double *__restrict__ bfull, double *__restrict__ M, unsigned *__restrict__ bar, int nsync) {
  __shared__ double tile[NB][NB + 1];
  const int ntri = nt * (nt + 1) / 2, t = blockIdx.x, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  if (t >= ntri) {  // the right-hand side (row D) and the back-substitution's progress words
    const int j = (t - ntri) * 256 + threadIdx.x;
    if (j < nsync) bar[j] = 0u;
    if (j < D) M[(size_t)D * ld + j] = bfull[keep_index(j, gauge_axis)];
    return;
  }
  int I, J;
  tri_tile(t, I, J);
  const int i_in = NB * I + tx;  // this thread reads column gi(i_in) of the packed rows gj(j), j = 32 J + ty + 8 q
  const int gi = keep_index(min(i_in, D - 1), gauge_axis);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = NB * J + ty + 8 * q, gj = keep_index(min(j, D - 1), gauge_axis);
    tile[ty + 8 * q][tx] = packed_sym(Afull, m, gi, gj);  // (on a diagonal tile the upper elements read their mirror image; never stored)
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = NB * I + ty + 8 * q, j = NB * J + tx;
    if (i < D && j <= i) M[(size_t)i * ld + j] = tile[tx][ty + 8 * q];
  }
}

__device__ __forceinline__ double readlane_d(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// MFMA operands straight from row-major rows: the product sums over k, so any permutation of k
// that A and B share is allowed.  Lane (idx = l & 15, kq = l >> 4) loads the 4 CONSECUTIVE
// doubles X[idx][16 g + 4 kq .. + 3] (one 32-byte load; a row's 16-column group is one full
// 128-byte line across kq) and feeds element u to MFMA step 4 g + u (k_chol_trail32).

// One launch per 128-column super-block [jS, jE).  Workgroup = 5 waves: wave 0 runs the serial
// chain (the four 32x32 tile factorisations), waves 1..4 ("workers", 16 rows each) own 64 rows
// below the super-block and do all the MFMA work.  EVERY workgroup factors the whole 128x128
// diagonal block in LDS (redundant, but there is no inter-workgroup dependency inside the
// super-block, so its four panels need one dispatch instead of four).  Per 32-column panel q:
//   F  wave 0: lanes 0..31 keep row r of tile (q,q) in registers, lanes 32..63 row r of the
//      IDENTITY: the column operations of the factorisation (entries of L broadcast with
//      v_readlane: no LDS, every index static) turn the identity rows into L^-T (Zt, double-buffered)
//      workers, meanwhile: the updates of panel q-1 that the chain does not wait for
//      (T[r][c] -= X[r][q-1] X[c][q-1]^T for every tile but (q,q)), their own rows of panel q-1
//      (X = P L^-T -> global) and the left-looking update of their own rows for panel q
//      (P_q -= sum_{q'<q} X_q' L[q][q']^T, A operands kept in registers)
//   T  workers: in-block tiles (r,q), r > q: X = T L_qq^-T (in place)
//   U  workers: tile (q+1,q+1) -= X[q+1][q] X[q+1][q]^T  -- the only update on the critical path
// Workgroup 0 also writes the in-block X tiles (Lblk: this super-block's 128x128 row-major block)
// and the L^-T tiles (Ztiles) for the back-substitution to their OWN buffers: the diagonal block
// of M is never written, because other workgroups may still be loading it.
// MFMA layouts: A/B lane l holds X[idx = l & 15][k = 16 g + 4 (l >> 4) + u] at step (g, u)
// (the k-permutation above); C/D: col = l & 15, row = (l >> 4) + 4 reg.
constexpr int TS = NB + 1;                               // padded LDS tile row stride
constexpr int SUPER_THREADS = 384;  // waves 0..5: chain, workers 0..2, an idle wave (keeps the chain alone on its SIMD), worker 3
constexpr int SUPER_LDS = (12 * NB * TS + 64 * TS + 64 * 9) * 8;  // 10 tiles + 2 Zt + Pt + panel buffer, bytes
constexpr int BACKSOLVE_LDS = (11 * NB * TS + 5 * SBW) * 8;  // k_chol_backsolve_all: 10 tiles + a scratch tile + y + partial sums + x, bytes
// the 10 tiles of a super-block's lower block triangle, numbered row by row: (r, c <= r) <-> r (r + 1) / 2 + c
__device__ __forceinline__ int tix(int r, int c) { return r * (r + 1) / 2 + c; }
__device__ __forceinline__ void tix_rc(int t, int &r, int &c) {
  const int row = (t >= 6) ? 3 : (t >= 3) ? 2 : (t >= 1) ? 1 : 0;
  r = row;
  c = t - row * (row + 1) / 2;
}

// Tile factorisation on one wave (see F above); returns false if a pivot is not positive.
// The augmented 64x32 matrix B = [tile; I] (column operations turn it into [L; L^-T]) lives in
// MFMA C/D layout (acc[row tile][column tile]).  Per panel of 8 columns:
//   a. the panel's columns go through LDS (Xb) into a row-per-lane register block bp[8]
//   b. 8 elimination steps restricted to the panel: 28 v_readlane broadcasts instead of ~200
//   c. bp back to Xb (and the L^-T rows to Zt)
//   d. every later column at once: acc -= B[:, panel] L[cols, panel]^T as f64 MFMAs whose A and
//      B operands are both read from Xb (B operand of column tile ct = A operand of row tile ct)
// 112 broadcast-FMAs + 32 MFMAs instead of 496 broadcast-FMAs: ~21k -> ~10k cycles per tile.
constexpr int XBS = 9;  // padded row stride of the 64 x 8 panel buffer
__device__ __forceinline__ bool factor_tile(const double (*tile)[TS], double (*Zt)[TS], double *Xb, int lane, bool store,
                                            double *__restrict__ Ztile, int nvalid) {
  const int li = lane & 15, lk = lane >> 4;
  mvba_d4 acc[4][2];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 16 * (rt & 1) + lk + 4 * q, col = 16 * ct + li;
        acc[rt][ct][q] = (rt < 2) ? tile[row][col] : ((row == col) ? 1.0 : 0.0);
      }
  bool bad = false;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    // a. panel columns 8p .. 8p+7: C/D layout -> one row per lane
    if ((li >> 3) == (p & 1)) {
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int q = 0; q < 4; ++q) Xb[(16 * rt + lk + 4 * q) * XBS + (li & 7)] = acc[rt][p >> 1][q];
    }
    wave_sync();
    double bp[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bp[j] = Xb[lane * XBS + j];
    // b. elimination inside the panel
    // Two pivots per step: with a = B[k][k], b = B[k+1][k], c = B[k+1][k+1] the two reciprocal roots
    // 1/l11 = rsq(a) and 1/l22 = rsq(a c - b^2) * l11 do not depend on each other, so the serial chain
    // (rsq + two Newton steps + broadcast) is walked 16 times per tile instead of 32.  a c - b^2
    // loses the same digits as the usual c - b^2 / a (both are det / a up to the factor a).
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
      const int r0 = 8 * p + k, r1 = r0 + 1;
      const double a = readlane_d(bp[k], r0), b = readlane_d(bp[k], r1), c = readlane_d(bp[k + 1], r1);
      const double det = fma(a, c, -b * b);
      bad |= !(a > 0.0) | !(det > 0.0);
      double ra = __builtin_amdgcn_rsq(a), rd = __builtin_amdgcn_rsq(det);
      ra = ra * (1.5 - 0.5 * a * ra * ra);
      rd = rd * (1.5 - 0.5 * det * rd * rd);
      ra = ra * (1.5 - 0.5 * a * ra * ra);
      rd = rd * (1.5 - 0.5 * det * rd * rd);
      const double l21 = b * ra, inv22 = rd * (a * ra);
      bp[k] = bp[k] * ra;
      bp[k + 1] = (bp[k + 1] - bp[k] * l21) * inv22;
#pragma unroll
      for (int j = k + 2; j < 8; ++j)
        bp[j] -= bp[k] * readlane_d(bp[k], 8 * p + j) + bp[k + 1] * readlane_d(bp[k + 1], 8 * p + j);
    }
    // c. finished columns back to Xb; rows 32..63 are rows of L^-T
#pragma unroll
    for (int j = 0; j < 8; ++j) Xb[lane * XBS + j] = bp[j];
    if (lane >= 32) {
      const int r = lane - 32;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = 8 * p + j;
        Zt[r][c] = bp[j];
        if (store && r < nvalid && c >= r && c < nvalid) Ztile[r * NB + c] = bp[j];
      }
    }
    // d. all later columns: acc[rt][ct] -= B[16 rt .., panel] L[16 ct .., panel]^T
    wave_sync();
    if (p < 3) {
      double xa[4][2];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int t = 0; t < 2; ++t) xa[rt][t] = Xb[(16 * rt + li) * XBS + 4 * t + lk];
#pragma unroll
      for (int ct = (p == 0) ? 0 : 1; ct < 2; ++ct)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int t = 0; t < 2; ++t)
            acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa[rt][t], xa[ct][t], acc[rt][ct], 0, 0, 0);
      wave_sync();  // the next panel overwrites Xb
    }
  }
  return !bad;
}

__device__ __forceinline__ void chol_super_body(double *lds, double *M, int ld, int D, int jS, double *__restrict__ Ztiles,
                                                double *__restrict__ Lblk, int *__restrict__ flag, int bid) {
  double (*T)[NB][TS] = reinterpret_cast<double (*)[NB][TS]>(lds);
  double (*Zt)[NB][TS] = reinterpret_cast<double (*)[NB][TS]>(lds + 10 * NB * TS);
  double (*Pt)[TS] = reinterpret_cast<double (*)[TS]>(lds + 12 * NB * TS);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ww = (wave == 0 || wave == 4) ? -1 : (wave == 5 ? 3 : wave - 1);  // worker index (chain and idle waves: -1)
  const int li = lane & 15, lk = lane >> 4;
  const int nbS = min(SBW, D - jS), jE = jS + nbS, nq = (nbS + NB - 1) / NB;
  const int R0 = jE + bid * 64 + 16 * ww;  // this worker's first row below the super-block
  const bool wg0 = bid == 0;
  const mvba_d4 zero4 = {0.0, 0.0, 0.0, 0.0};
  // Loads, in the order they are needed (one CU draws ~25 GB/s from beyond its L2, so the 144 KiB a
  // workgroup needs take ~8 us: the chain must not wait for all of it):
  //   1. diagonal tile (0,0), by every thread -> LDS -> barrier: wave 0 starts factoring it
  //   2. the workers' own rows of all four panels (C/D layout; consumed panel by panel) and the other
  //      nine tiles of the diagonal block, by waves 1..5: in LDS before barrier B1 of panel 0
  // (lower block triangle; identity padding beyond nbS).  The loads are UNCONDITIONAL on clamped
  // addresses: behind a lane-dependent branch the compiler cannot count how many loads are in flight
  // and waits for all of them (vmcnt(0)) at the first use.
  // (the selection is done on the bit pattern: written as "cond ? loaded : other" the compiler sinks
  // the load back under the branch)
  auto pick = [](bool c, double loaded, double other) -> double {
    const long long m = c ? -1LL : 0LL;
    return __longlong_as_double((__double_as_longlong(loaded) & m) | (__double_as_longlong(other) & ~m));
  };
  // tile_raw requests an element, tile_fix (at the point of use, so that no wait is scheduled
  // earlier) replaces what lies outside the lower triangle / the matrix by the identity padding
  auto tile_raw = [&](int t, int idx) -> double {
    int r, c;
    tix_rc(t, r, c);
    const int i = idx >> 5, j = idx & 31, gi = NB * r + i, gj = NB * c + j, gic = min(gi, nbS - 1);
    return M[(size_t)(jS + gic) * ld + jS + min(gj, gic)];
  };
  auto tile_fix = [&](int t, int idx, double raw) -> double {
    int r, c;
    tix_rc(t, r, c);
    const int i = idx >> 5, j = idx & 31, gi = NB * r + i, gj = NB * c + j;
    return pick(idx < NB * NB && gi < nbS && gj <= gi, raw, (gi == gj) ? 1.0 : 0.0);
  };
  constexpr int P0 = (NB * NB + SUPER_THREADS - 1) / SUPER_THREADS;
  constexpr int RT = SUPER_THREADS - 64, PR = (NB * NB + RT - 1) / RT;  // the rest: every wave but the chain
  double v0[P0];
#pragma unroll
  for (int ps = 0; ps < P0; ++ps) v0[ps] = tile_raw(0, tid + ps * SUPER_THREADS);
  auto store_tile0 = [&]() {
#pragma unroll
    for (int ps = 0; ps < P0; ++ps) {
      const int idx = tid + ps * SUPER_THREADS;
      if (idx < NB * NB) T[0][idx >> 5][idx & 31] = tile_fix(0, idx, v0[ps]);
    }
    __syncthreads();  // tile (0,0) loaded
  };
  if (wave == 0) {
    // ---- the chain: nothing else to load (its own code path, so that its wait counts only its loads)
    store_tile0();
    for (int q = 0; q < nq; ++q) {
      // ---- F
      const bool ok = factor_tile(T[tix(q, q)], Zt[q & 1], lds + 12 * NB * TS + 64 * TS, lane, wg0, Ztiles + (size_t)q * NB * NB, nbS - NB * q);
      if (!ok && wg0 && lane == 0) atomicOr(flag, FLAG_NOT_POSDEF);
      __syncthreads();  // B1: Zt[q & 1] ready; tiles (r,q), r > q, final
      __syncthreads();  // B2: X tiles of panel q complete
      __syncthreads();  // B3: tile (q+1,q+1) final
    }
    return;
  }
  // ---- workers (and the idle wave): tile (0,0) first, so that the chain starts after ONE short round
  // trip; their own loads follow in one batch and have the ~7 us of the first tile factorisation to land
  store_tile0();
  double P[4][4][2];
  double vr[9][PR];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {  // (the idle wave loads a clamped dummy row group like a worker)
      const double *src = M + (size_t)min(max(R0 + lk + 4 * qq, 0), D) * ld + jS;
      P[q][qq][0] = src[min(NB * q + li, nbS - 1)];
      P[q][qq][1] = src[min(NB * q + 16 + li, nbS - 1)];
    }
#pragma unroll
  for (int t = 1; t < 10; ++t)
#pragma unroll
    for (int ps = 0; ps < PR; ++ps) vr[t - 1][ps] = tile_raw(t, tid - 64 + ps * RT);
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int row = R0 + lk + 4 * qq;
      P[q][qq][0] = pick(ww >= 0 && row <= D && NB * q + li < nbS, P[q][qq][0], 0.0);
      P[q][qq][1] = pick(ww >= 0 && row <= D && NB * q + 16 + li < nbS, P[q][qq][1], 0.0);
    }
#pragma unroll
  for (int t = 1; t < 10; ++t)
#pragma unroll
    for (int ps = 0; ps < PR; ++ps) {
      const int idx = tid - 64 + ps * RT;
      if (idx < NB * NB) T[t][idx >> 5][idx & 31] = tile_fix(t, idx, vr[t - 1][ps]);
    }
  mvba_d4 XA[3][2];  // own rows' X of the earlier panels, A layout
#pragma unroll
  for (int q = 0; q < 3; ++q) XA[q][0] = XA[q][1] = zero4;

  // own rows of panel q: X = P Zt, store, and keep X in A layout (through this worker's slice of Pt) for the later panels
  auto own_trsm = [&](int q, mvba_d4 &xa0, mvba_d4 &xa1) {
    const double (*Z)[TS] = Zt[q & 1];
    mvba_d4 x0 = zero4, x1 = zero4;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = 16 * g + 4 * lk + u;
        const double av = Pt[16 * ww + li][k];
        if (g == 0) x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Z[k][li], x0, 0, 0, 0);
        x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Z[k][16 + li], x1, 0, 0, 0);
      }
    wave_sync();  // every lane has read its operands out of this slice of Pt
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int row = R0 + lk + 4 * qq;
      if (row <= D) {
        double *dst = M + (size_t)row * ld + jS + NB * q;
        if (NB * q + li < nbS) dst[li] = x0[qq];
        if (NB * q + 16 + li < nbS) dst[16 + li] = x1[qq];
      }
      Pt[16 * ww + lk + 4 * qq][li] = x0[qq];
      Pt[16 * ww + lk + 4 * qq][16 + li] = x1[qq];
    }
    wave_sync();  // C/D layout written by some lanes, A layout read by others
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      xa0[u] = Pt[16 * ww + li][4 * lk + u];
      xa1[u] = Pt[16 * ww + li][16 + 4 * lk + u];
    }
  };
  // 16x16 sub-tile (ih, jh) of T[r][c] -= X[r][q] X[c][q]^T
  auto update_sub = [&](int r, int c, int q, int ih, int jh) {
    mvba_d4 acc = zero4;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = 16 * g + 4 * lk + u;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(T[tix(r, q)][16 * ih + li][k], T[tix(c, q)][16 * jh + li][k], acc, 0, 0, 0);
      }
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) T[tix(r, c)][16 * ih + lk + 4 * qq][16 * jh + li] -= acc[qq];
  };

  // Role split by whole waves (every role executes the same number of workgroup barriers per
  // panel: F | B1 | T | B2 | U | B3).  Separate code paths keep the chain's registers (a tile row)
  // and the workers' registers (own rows, A operands) out of each other's live ranges.
  if (ww < 0) {  // the idle wave (the chain returned above)
    for (int q = 0; q < nq; ++q) {
      __syncthreads();
      __syncthreads();
      __syncthreads();
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q >= nq) break;  // uniform
    // ---- F (while wave 0 factors tile (q,q))
    if (q > 0) {
      int sidx = 0;  // panel q-1's updates of every tile but (q,q)
      for (int r = q; r < nq; ++r)
        for (int c = q; c <= r; ++c) {
          if (r == q && c == q) continue;
          for (int sub = 0; sub < 4; ++sub) {
            const int ih = sub >> 1, jh = sub & 1;
            if (r == c && jh > ih) continue;  // upper sub-tile of a diagonal tile: never read
            if ((sidx++ & 3) == ww) update_sub(r, c, q - 1, ih, jh);
          }
        }
      own_trsm(q - 1, XA[q - 1][0], XA[q - 1][1]);
    }
    {  // own rows: left-looking update of panel q, result to this worker's slice of Pt
      mvba_d4 acc0 = zero4, acc1 = zero4;
#pragma unroll
      for (int qp = 0; qp < q; ++qp)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = 16 * g + 4 * lk + u;
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(XA[qp][g][u], T[tix(q, qp)][li][k], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(XA[qp][g][u], T[tix(q, qp)][16 + li][k], acc1, 0, 0, 0);
          }
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        Pt[16 * ww + lk + 4 * qq][li] = P[q][qq][0] - acc0[qq];
        Pt[16 * ww + lk + 4 * qq][16 + li] = P[q][qq][1] - acc1[qq];
      }
    }
    __syncthreads();  // B1
    // ---- T: in-block tiles (r,q): X = T Zt in place, one 16-row unit per worker at a time
    {
      const double (*Z)[TS] = Zt[q & 1];
      for (int e = ww; e < 2 * (nq - 1 - q); e += 4) {
        const int r = q + 1 + (e >> 1), h = e & 1;
        double (*tile)[TS] = T[tix(r, q)];
        double av[2][4];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int u = 0; u < 4; ++u) av[g][u] = tile[16 * h + li][16 * g + 4 * lk + u];
        mvba_d4 x0 = zero4, x1 = zero4;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = 16 * g + 4 * lk + u;
            if (g == 0) x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[g][u], Z[k][li], x0, 0, 0, 0);
            x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[g][u], Z[k][16 + li], x1, 0, 0, 0);
          }
        wave_sync();  // in place: every lane has read its operands before any lane overwrites the unit
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int i = 16 * h + lk + 4 * qq;
          tile[i][li] = x0[qq];
          tile[i][16 + li] = x1[qq];
          if (wg0 && NB * r + i < nbS) {  // columns of panel q are all < nbS here (q < r)
            double *dst = Lblk + (size_t)(NB * r + i) * SBW + NB * q;
            dst[li] = x0[qq];
            dst[16 + li] = x1[qq];
          }
        }
      }
    }
    __syncthreads();  // B2
    // ---- U: the next diagonal tile, three 16x16 sub-tiles on three workers
    if (q + 1 < nq && ww < 3) update_sub(q + 1, q + 1, q, ww == 0 ? 0 : 1, ww == 2 ? 1 : 0);
    __syncthreads();  // B3
  }
  {  // own rows of the last panel
    mvba_d4 d0, d1;
    own_trsm(nq - 1, d0, d1);
  }
}

__global__ __launch_bounds__(SUPER_THREADS) void k_chol_super(double *M, int ld, int D, int jS, double *__restrict__ Ztiles,
                                                              double *__restrict__ Lblk, int *__restrict__ flag) {
  extern __shared__ double lds[];
  chol_super_body(lds, M, ld, D, jS, Ztiles, Lblk, flag, blockIdx.x);
}

// Trailing update with f64 MFMA for the finished super-block [jS, jE): C -= P P^T on rows/cols
// >= jE (jE - jS == SBW).  One workgroup per 32 x 32 tile of the lower triangle, the K = 128 columns
// split over its four waves (32 each) and the four partial tiles summed through LDS: 72 KiB of operands
// per workgroup, and one CU draws only ~25 GB/s from beyond its L2, so many small workgroups spread the loads.
__global__ __launch_bounds__(256) void k_chol_trail32(double *M, int ld, int D, int jS, int jE) {
  __shared__ double part[4][NB][NB + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  int by, bx;  // this workgroup's tile of the lower triangle
  tri_tile(blockIdx.x, by, bx);
  const int r0 = jE + NB * by, c0 = jE + NB * bx;
  // C (this thread's four elements), requested first
  double cv[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = threadIdx.x + 256 * q, rr = r0 + (e >> 5), cc = c0 + (e & 31);
    cv[q] = M[(size_t)min(rr, D) * ld + min(cc, D - 1)];
  }
  mvba_d4 av[2][2], bv[2][2];  // [row group of 16][k group of 16]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      av[i][g] = *reinterpret_cast<const mvba_d4 *>(M + (size_t)min(r0 + 16 * i + li, D) * ld + jS + 32 * wave + 16 * g + 4 * lk);
      bv[i][g] = *reinterpret_cast<const mvba_d4 *>(M + (size_t)min(c0 + 16 * i + li, D) * ld + jS + 32 * wave + 16 * g + 4 * lk);
    }
  mvba_d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = mvba_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i][g][u], bv[j][g][u], acc[i][j], 0, 0, 0);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) part[wave][16 * i + lk + 4 * q][16 * j + li] = acc[i][j][q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = threadIdx.x + 256 * q, i = e >> 5, j = e & 31, rr = r0 + i, cc = c0 + j;
    const double sum = (part[0][i][j] + part[1][i][j]) + (part[2][i][j] + part[3][i][j]);
    if (rr <= D && cc < D && cc <= rr) M[(size_t)rr * ld + cc] = cv[q] - sum;
  }
}

// The same update for LARGE trailing matrices: k_chol_trail32 reads 64 KiB of operands per 32 x 32 tile straight into
// registers -- every tile of a tile row re-reads that row's 32 x 128 panel from L2.  Here a workgroup owns 64 x 64 of C (four
// waves, 32 x 32 each), the K = 128 columns stream through LDS in chunks of 16 (A and B chunk 8 KiB each, double-buffered, the
// next chunk's global loads in flight during the MFMAs of this one): 32 KiB of operands per 32 x 32 of C instead of 64, one
// batch of C loads that lands during the loop, four workgroups per CU in different phases (hence the launch bound).
// Diagonal workgroups compute the full square and store the lower triangle (their upper-right wave only keeps the barriers
// company).  Below ~200 workgroups k_chol_trail32 wins: a workgroup here lives >= 8 us, there 2-5 (the host's trail64_min;
// measurements and the rejected 128 x 128 tile: DESIGN.md 3.2 and 3.3).
constexpr int TB = 64, TB_KC = 16, TB_LD = TB_KC + 2;                  // tile, chunk of K, padded LDS row (144 bytes: 16-byte aligned)
constexpr int TRAIL64_LDS = 2 * 2 * TB * TB_LD * (int)sizeof(double);  // 2 buffers x (A, B): 36,864 bytes
__global__ __launch_bounds__(256, 4) void k_chol_trail64(double *M, int ld, int D, int jS, int jE) {
  extern __shared__ double lds[];
  double (*As)[TB][TB_LD] = reinterpret_cast<double (*)[TB][TB_LD]>(lds);
  double (*Bs)[TB][TB_LD] = reinterpret_cast<double (*)[TB][TB_LD]>(lds + 2 * TB * TB_LD);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4, wy = wave >> 1, wx = wave & 1;
  int by, bx;
  tri_tile(blockIdx.x, by, bx);
  const int r0 = jE + TB * by, c0 = jE + TB * bx;
  const bool idle = (bx == by) && wy == 0 && wx == 1;  // entirely above the diagonal
  // this thread's share of a chunk: 4 consecutive doubles of one row of A and of B (four threads per 128-byte line)
  const int prow = tid >> 2, pcol = 4 * (tid & 3);
  const double *asrc = M + (size_t)min(r0 + prow, D) * ld + jS + pcol;
  const double *bsrc = M + (size_t)min(c0 + prow, D) * ld + jS + pcol;
  mvba_d4 pa = *reinterpret_cast<const mvba_d4 *>(asrc), pb = *reinterpret_cast<const mvba_d4 *>(bsrc);
  // C (C/D layout: col = li, row = lk + 4 q): requested now, needed after the loop
  double cv[2][2][4];
#pragma unroll
  for (int rg = 0; rg < 2; ++rg)
#pragma unroll
    for (int cg = 0; cg < 2; ++cg)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        cv[rg][cg][q] = M[(size_t)min(r0 + 16 * (2 * wy + rg) + lk + 4 * q, D) * ld + min(c0 + 16 * (2 * wx + cg) + li, D - 1)];
  mvba_d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = mvba_d4{0.0, 0.0, 0.0, 0.0};
  auto stage = [&](int b) {
    *reinterpret_cast<mvba_d4 *>(&As[b][prow][pcol]) = pa;
    *reinterpret_cast<mvba_d4 *>(&Bs[b][prow][pcol]) = pb;
  };
  stage(0);
  __syncthreads();
#pragma unroll 1
  for (int g = 0; g < SBW / TB_KC; ++g) {
    const int b = g & 1;
    if (g + 1 < SBW / TB_KC) {
      pa = *reinterpret_cast<const mvba_d4 *>(asrc + TB_KC * (g + 1));
      pb = *reinterpret_cast<const mvba_d4 *>(bsrc + TB_KC * (g + 1));
    }
    if (!idle) {
      // lane (li, lk) holds X[16 rg + li][4 lk + u] for MFMA step u: the k-permutation both operands share (see above)
      mvba_d4 av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        av[i] = *reinterpret_cast<const mvba_d4 *>(&As[b][16 * (2 * wy + i) + li][4 * lk]);
        bv[i] = *reinterpret_cast<const mvba_d4 *>(&Bs[b][16 * (2 * wx + i) + li][4 * lk]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int rg = 0; rg < 2; ++rg)
#pragma unroll
          for (int cg = 0; cg < 2; ++cg) acc[rg][cg] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rg][u], bv[cg][u], acc[rg][cg], 0, 0, 0);
    }
    if (g + 1 < SBW / TB_KC) stage(b ^ 1);  // (read by compute(g - 1): every wave is past it since the barrier below)
    __syncthreads();
  }
  if (idle) return;
#pragma unroll
  for (int rg = 0; rg < 2; ++rg)
#pragma unroll
    for (int cg = 0; cg < 2; ++cg)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = r0 + 16 * (2 * wy + rg) + lk + 4 * q, cc = c0 + 16 * (2 * wx + cg) + li;
        if (rr <= D && cc < D && cc <= rr) M[(size_t)rr * ld + cc] = cv[rg][cg][q] - acc[rg][cg][q];
      }
}

// One tile of the back-substitution inside a super-block, for both forms below (tiles walked from the bottom, t = 3 .. 0):
// x_t = Z_t y_t, a 32 x 32 mat-vec on wave 0 (Z_t = L_tt^-T from k_chol_super: no serial substitution).  ys: the block's y,
// turning into x from the bottom; nb: rows of x_t to write.  The caller has Z_t and ys complete before the call, and follows it
// with a barrier and its own y[c] -= sum_r L[32 t + r][c] x_t[r] for the columns c < 32 t (the forms keep L in different places).
__device__ __forceinline__ void backsolve_tile_x(const double (*Z)[TS], double *ys, int t, int nb, int lane, int wave) {
  if (wave == 0) {
    const int r = lane & 31, h = lane >> 5;  // two lanes per row, 16 columns each
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int q = 0; q < NB / 2; q += 2) {
      s0 += Z[r][16 * h + q] * ys[t * NB + 16 * h + q];
      s1 += Z[r][16 * h + q + 1] * ys[t * NB + 16 * h + q + 1];
    }
    double xr = s0 + s1;
    xr += __shfl_xor(xr, 32, 64);
    if (lane < nb) ys[t * NB + lane] = xr;  // all reads of ys above precede this write (one wave, in order)
  }
}

// L^T x = y (y = row D of M, overwritten by x), one launch per 128-column super-block, last one
// first.  Launch for super-block [jS, jE), given the finished x of the super-block above it
// [jE, jE2):
//   workgroups >= 1   y[c] -= sum_r L[r][c] x[r]  (r in [jE, jE2)) for the columns c < jS, one column
//                     per thread, rows read coalesced: the bulk of the memory traffic, chip-wide
//   workgroup 0       the same for its own columns [jS, jE), then the four tiles from the bottom (backsolve_tile_x; Z_t from
//                     Ztiles, the in-block L from Lblk, see k_chol_super);
//                     scatters x into the full 9m vector (zeros at the gauge slots).
// Always launched with 256 threads.
__global__ __launch_bounds__(256) void k_chol_backsolve(double *M, int ld, int D, int m, int gauge_axis,
                                                        const double *__restrict__ Ztiles, const double *__restrict__ Lblk,
                                                        double *__restrict__ dxi_full, int jS, int jE, int jE2) {
  __shared__ double xp[SBW];  // x of the super-block above
  __shared__ double ys[SBW];  // y, then x, of this super-block
  __shared__ double part[2][SBW];
  __shared__ double T[NB][NB + 1];
  const int bid = blockIdx.x, tid = threadIdx.x;
  double *y = M + (size_t)D * ld;
  const int np = jE2 - jE;  // 0 for the first launch (top super-block)
  if (tid < SBW) xp[tid] = (tid < np) ? y[jE + tid] : 0.0;
  __syncthreads();
  if (bid > 0) {
    const int c = (bid - 1) * 256 + tid;
    if (c < jS) {
      const double *col = M + (size_t)jE * ld + c;
      double s0 = 0.0, s1 = 0.0;
      int r = 0;
      for (; r + 16 <= np; r += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = col[(size_t)(r + u) * ld];
#pragma unroll
        for (int u = 0; u < 16; u += 2) {
          s0 += v[u] * xp[r + u];
          s1 += v[u + 1] * xp[r + u + 1];
        }
      }
      for (; r < np; ++r) s0 += col[(size_t)r * ld] * xp[r];
      y[c] -= s0 + s1;
    }
    return;
  }
  const int ns = jE - jS;
  {
    const int c = tid & (SBW - 1), h = tid >> 7;  // two threads per column, alternate rows
    double s = 0.0;
    if (c < ns) {
      const double *col = M + (size_t)jE * ld + jS + c;
#pragma unroll 8
      for (int r = h; r < np; r += 2) s += col[(size_t)r * ld] * xp[r];
    }
    part[h][c] = s;
    __syncthreads();
    if (tid < SBW) ys[tid] = (tid < ns) ? y[jS + tid] - part[0][tid] - part[1][tid] : 0.0;
    if (np == 0)  // first launch on the stream: clear the gauge slots before any x is scattered
      for (int i = tid; i < 9 * m; i += 256) dxi_full[i] = 0.0;
    __syncthreads();
  }
  for (int t = (ns + NB - 1) / NB - 1; t >= 0; --t) {
    const int jb = jS + t * NB, nb = min(NB, jE - jb);
    for (int q = tid; q < NB * NB; q += 256) {
      const int r = q / NB, c = q % NB;
      T[r][c] = (r < nb && c >= r && c < nb) ? Ztiles[(size_t)(jb / NB) * NB * NB + q] : 0.0;
    }
    // operands of this tile's update inside the super-block, one column per thread
    double lcol[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) lcol[r] = (tid < t * NB && r < nb) ? Lblk[(size_t)(t * NB + r) * SBW + tid] : 0.0;
    __syncthreads();
    backsolve_tile_x(T, ys, t, nb, tid & 63, tid >> 6);
    __syncthreads();
    if (tid < t * NB) {
      double sacc = 0.0;
#pragma unroll
      for (int r = 0; r < NB; ++r) sacc += lcol[r] * ys[t * NB + r];  // lcol = 0 beyond nb
      ys[tid] -= sacc;
    }
    __syncthreads();
  }
  if (tid < ns) {
    y[jS + tid] = ys[tid];
    dxi_full[keep_index(jS + tid, gauge_axis)] = ys[tid];
  }
}

// Hand-overs between the workgroups of a persistent grid (every workgroup co-resident: at most one per CU), point to point:
// thread 0 of a workgroup waits until a progress word has reached `target` (words only grow).  No device-wide
// fences: an agent-scope release / acquire pair is a write-back / invalidate of the whole L2 of the XCD (1.7 + 1.5 us of an
// 11.6 us chain step with 140 workgroups doing the same, profiles/r04_backsolve_chain_trace_d4493.txt), and the only
// data that travels between workgroups here is the vector y.  So every access to y inside this kernel is an agent-scope
// atomic (sc1: stores write through to memory, loads do not hit a stale line), a producer's waves wait for their stores
// (s_waitcnt vmcnt(0)), meet at a barrier, and then thread 0 stores the word; the consumer polls it,
// passes a barrier and loads.  A wait gives up after `max_polls` polls (2^22 by default), and at once when somebody else already
// has: FLAG_WAIT_GAVE_UP, the host redoes the solve with one launch per super-block.  So the grid always drains.
template <int SLEEP>
__device__ __forceinline__ void flow_wait(const unsigned *word, unsigned target, int *flag, unsigned max_polls) {
  unsigned spins = 0;
  while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
    __builtin_amdgcn_s_sleep(SLEEP);
    ++spins;
    if (spins > max_polls || ((spins & 127u) == 0u && (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & FLAG_WAIT_GAVE_UP))) {
      atomicOr(flag, FLAG_WAIT_GAVE_UP);
      break;
    }
  }
}
__device__ __forceinline__ void flow_post(unsigned *word, unsigned value) {
  // this wave's sc1 stores have COMPLETED before anybody stores the word: a workgroup-scope release fence is not enough (in
  // this execution mode the compiler lowers it to nothing -- waves of a workgroup share their L1 -- and the word would chase
  // the data through different L2 channels), hence the explicit wait
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double flow_load(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void flow_store(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- L^T x = y for all super-blocks in ONE persistent launch (last block first) instead of S launches.  Step s (x_{s+1} known):
//   workgroup s ("chain" of block s)
//       y_s -= (rows of the block above)^T x_{s+1}; then the block's four tiles from the bottom:
//       x_t = Z_t y_t (Z = L_tt^-T from the factorisation), y_{t' < t} -= L[t][t']^T x_t.
//       Everything static it needs (Z tiles and in-block L tiles -> LDS, the 128 x 128 panel below the
//       block -> registers: 208 KiB, ~10 us for one CU) is loaded when the kernel starts, by all S chain
//       workgroups at once; at its step a chain workgroup reads only x_{s+1} and y_s (2 KiB).
//   workgroups >= S ("bulk")
//       y[c] -= (rows of block s+1)^T x_{s+1} for the columns left of block s, 32 columns x 8 row
//       chunks per workgroup: one batch of 16 loads per thread, LDS reduction.
// x_s must reach the next chain and the bulk workgroups, their updates the chain, with no device-wide barrier.  sync[0] = number of x blocks published (chain s posts S - s);
// sync[1 + g] = number of x blocks applied to the 32-column group g, whose owner among the bulk workgroups applies them
// last block first.  Chain s waits for x_{s+1} and for x_{s+2} on its own four groups -- applied a whole chain step
// earlier, so it practically never waits for the bulk -- and a bulk workgroup for the x it is about to apply.  With nobody
// else in a barrier the bulk can be one workgroup per group (140 at D = 4493 instead of 16: 11 us of a 14 us step were
// their share of the matrix at ~25 GB/s each).
// (FLOW = true is the only form.  The parameter stays so that the kernel keeps the symbol csrc/check_isa.py, the tests and
// the committed kernel profiles name: k_chol_backsolve_all<true>.)
template <bool FLOW>
__global__ __launch_bounds__(SUPER_THREADS) void k_chol_backsolve_all(double *M, int ld, int D, int m, int gauge_axis,
                                                                      const double *Ztiles, const double *Lblk_all, double *dxi_full,
                                                                      int *flag, unsigned *bar, unsigned max_polls) {
  static_assert(FLOW, "only the point-to-point form of the back-substitution exists");
  extern __shared__ double lds[];
  const int G = gridDim.x, bid = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double *y = M + (size_t)D * ld;
  const int S = (D + SBW - 1) / SBW;
  double (*Zs)[NB][TS] = reinterpret_cast<double (*)[NB][TS]>(lds);                // [4]
  double (*Ls)[NB][TS] = reinterpret_cast<double (*)[NB][TS]>(lds + 4 * NB * TS);  // [6]: in-block tile (r, c < r) at r (r - 1) / 2 + c
  double (*Tt)[TS] = reinterpret_cast<double (*)[TS]>(lds + 10 * NB * TS);        // scratch tile of the block inverse
  double *ys = lds + 11 * NB * TS, *part = ys + SBW, *xs = part + 3 * SBW;         // part[3][SBW]; bulk: red[8][32], then x
  if (bid < S) {
    // ================= chain of block s = bid
    const int s = bid, jS = s * SBW, jE = min(jS + SBW, D), jE2 = min(jE + SBW, D), ns = jE - jS, np = jE2 - jE;
    // ---- static operands, one batch.  Every load is "uniform base + one per-thread offset", so the
    // addresses live in SGPRs and the batch fits the register file.
    const double *Lblk = Lblk_all + (size_t)s * SBW * SBW;
    constexpr int NT = SUPER_THREADS, NPASS = (NB * NB + NT - 1) / NT, NPN = (SBW + 2) / 3;
    double zl[10][NPASS], pn[NPN];
#pragma unroll
    for (int tile = 0; tile < 10; ++tile) {
      // tiles 0..3: Z (upper triangle of L_tt^-T); 4..9: in-block L tile (tr, tc < tr)
      const int e = tile - 4, tr = (e >= 3) ? 3 : (e >= 1) ? 2 : 1, tc = e - tr * (tr - 1) / 2;
      const double *base = (tile < 4) ? Ztiles + (size_t)(jS / NB + tile) * NB * NB : Lblk + (size_t)(NB * tr) * SBW + NB * tc;
      const int nb = ns - NB * (tile < 4 ? tile : tr);  // valid rows (and columns, for Z) of the tile
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps) {
        const int w = tid + NT * ps, r = w >> 5, c = w & 31;
        const bool ok = w < NB * NB && r < nb && (tile >= 4 || (c >= r && c < nb));
        zl[tile][ps] = ok ? base[tile < 4 ? w : r * SBW + c] : 0.0;
      }
    }
    const int pc = tid & (SBW - 1), ph = tid >> 7;  // three threads per column, every third row
    const int poff = ph * ld + pc;
#pragma unroll
    for (int i = 0; i < NPN; ++i) {
      const double *rowbase = M + (size_t)(jE + 3 * i) * ld + jS;  // uniform
      pn[i] = (pc < ns && ph + 3 * i < np) ? rowbase[poff] : 0.0;
    }
#pragma unroll
    for (int tile = 0; tile < 10; ++tile)
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps) {
        const int w = tid + NT * ps;
        if (w < NB * NB) Zs[tile][w >> 5][w & 31] = zl[tile][ps];  // Ls follows Zs: tile 4 + e lands in Ls[e]
      }
    // ---- blocks with three chain steps of waiting ahead of them: the block's whole L_ss^-T instead of a walk over its
    // four tiles at the step (2.8 of 5.7 us, profiles/r04_backsolve_chain_trace_d4493.txt).  From x_r = Z_r (y_r - sum_{c > r} L_cr^T x_c):
    //   x_r = sum_{c >= r} W_rc y_c,  W_rr = Z_r,  W_rc = -Z_r sum_{r < k <= c} L_kr^T W_kc,
    // six off-diagonal tiles, each two MFMA passes (the sum into the scratch tile, then -Z_r times it) on four waves, one
    // 16 x 16 quarter each; W_rc lands in the slot of L_cr, which nobody needs any more in this order.
    const bool inverse = (S - 1 - s) >= 3;
    if (inverse) {
      __syncthreads();  // the tiles are in LDS
      const int li = lane & 15, lk = lane >> 4, qi = (wave >> 1) & 1, qj = wave & 1;  // waves 0..3: quarter (qi, qj)
      auto lslot = [](int tr, int tc) { return tr * (tr - 1) / 2 + tc; };
#pragma unroll 1
      for (int pair = 0; pair < 6; ++pair) {
        const int r = (pair == 0) ? 2 : (pair == 1 || pair == 3) ? 1 : 0, c = (pair < 3) ? 3 : (pair < 5) ? 2 : 1;
        if (wave < 4) {
          mvba_d4 acc = {0.0, 0.0, 0.0, 0.0};
          for (int k = r + 1; k <= c; ++k) {
            const double (*Lk)[TS] = Ls[lslot(k, r)];                         // L_kr: A = L_kr^T, A[i][kk] = L_kr[kk][i]
            const double (*Wk)[TS] = (k == c) ? Zs[c] : Ls[lslot(c, k)];       // W_kc (already in L_ck's slot), W_cc = Z_c
#pragma unroll
            for (int g = 0; g < 8; ++g) {
              const int kk = 4 * g + lk;
              acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Lk[kk][16 * qi + li], Wk[kk][16 * qj + li], acc, 0, 0, 0);
            }
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) Tt[16 * qi + lk + 4 * q][16 * qj + li] = acc[q];
        }
        __syncthreads();
        mvba_d4 w = {0.0, 0.0, 0.0, 0.0};
        if (wave < 4) {
#pragma unroll
          for (int g = 0; g < 8; ++g) {
            const int kk = 4 * g + lk;
            w = __builtin_amdgcn_mfma_f64_16x16x4f64(-Zs[r][16 * qi + li][kk], Tt[kk][16 * qj + li], w, 0, 0, 0);
          }
        }
        __syncthreads();  // every wave has read L_cr's slot (only pair (r, c) itself uses it from here on) and the scratch tile
        if (wave < 4) {
          double (*Wo)[TS] = Ls[lslot(c, r)];
#pragma unroll
          for (int q = 0; q < 4; ++q) Wo[16 * qi + lk + 4 * q][16 * qj + li] = w[q];
        }
        __syncthreads();
      }
      for (int e = tid; e < NB * TS; e += NT) (&Tt[0][0])[e] = 0.0;  // the scratch tile now stands in for the tiles left of the diagonal
    }
    // this thread's row of W, tile by tile (x = W y below: row tid & 127)
    const double *wrow[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int r = (tid & (SBW - 1)) >> 5, ii = tid & 31;
      wrow[ct] = (ct < r) ? &Tt[ii][0] : (ct == r) ? &Zs[r][ii][0] : &Ls[ct * (ct - 1) / 2 + r][ii][0];
    }
    // ---- wait for the step
    if (s < S - 1) {
      if (tid == 0) {
        if (s + 2 <= S - 1)  // (posted a whole chain step ago: checked first, while x_{s+1} is still on its way)
          for (int q = 0; q < 4; ++q) flow_wait<1>(bar + 1 + 4 * s + q, (unsigned)(S - (s + 2)), flag, max_polls);
        flow_wait<0>(bar, (unsigned)(S - 1 - s), flag, max_polls);
      }
      __syncthreads();
    }
    // x_{s+1} (published by chain s+1 before its progress word) and y_s (complete but for the panel's share)
    const double yv = (tid < ns) ? flow_load(y + jS + tid) : 0.0;
    // one sc1 load per element of x_{s+1}, the rest reads LDS (43 sc1 loads per thread: 2.2 us of a step)
    if (tid < SBW) xs[tid] = (tid < np) ? flow_load(y + jE + tid) : 0.0;
    __syncthreads();
    double sa = 0.0, sb = 0.0;
    if (np > 0) {
      double xv[NPN];
#pragma unroll
      for (int i = 0; i < NPN; ++i) xv[i] = (ph + 3 * i < np) ? xs[ph + 3 * i] : 0.0;
#pragma unroll
      for (int i = 0; i + 1 < NPN; i += 2) {
        sa += pn[i] * xv[i];
        sb += pn[i + 1] * xv[i + 1];
      }
      if (NPN & 1) sa += pn[NPN - 1] * xv[NPN - 1];
    }
    part[ph * SBW + pc] = sa + sb;
    __syncthreads();
    if (tid < SBW) ys[tid] = (tid < ns) ? yv - part[tid] - part[SBW + tid] - part[2 * SBW + tid] : 0.0;
    __syncthreads();
    if (inverse) {  // x = W y: row i = tid & 127, the columns c with c % 3 == tid / 128
      // (tile bases per thread, the column offsets compile-time constants -- one code path per third: 86 LDS reads with
      // immediate offsets and 43 FMAs; with the addresses computed per element this took as long as the walk it replaces)
      auto row_dot = [&](auto PH) {
        constexpr int ph0 = decltype(PH)::value;
        double sacc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < NPN; ++k) {
          const int c = ph0 + 3 * k;
          if (c < SBW) sacc[k & 3] += wrow[c >> 5][c & 31] * ys[c];
        }
        return (sacc[0] + sacc[1]) + (sacc[2] + sacc[3]);
      };
      const double dot = ph == 0 ? row_dot(std::integral_constant<int, 0>{}) : ph == 1 ? row_dot(std::integral_constant<int, 1>{}) : row_dot(std::integral_constant<int, 2>{});
      part[ph * SBW + (tid & (SBW - 1))] = dot;
      __syncthreads();
      if (tid < SBW) ys[tid] = part[tid] + part[SBW + tid] + part[2 * SBW + tid];
      __syncthreads();
    } else
    // ---- the tile chain
    for (int t = (ns + NB - 1) / NB - 1; t >= 0; --t) {
      backsolve_tile_x(Zs[t], ys, t, NB, lane, wave);  // (nb = NB: rows beyond the block's end have a zero row in Zs -> 0)
      __syncthreads();
      if (tid < t * NB) {
        const double (*Lt)[TS] = Ls[t * (t - 1) / 2 + (tid >> 5)];
        double sacc = 0.0;
#pragma unroll
        for (int r = 0; r < NB; ++r) sacc += Lt[r][tid & 31] * ys[t * NB + r];
        ys[tid] -= sacc;
      }
      __syncthreads();
    }
    if (tid < ns) {
      flow_store(y + jS + tid, ys[tid]);
      dxi_full[keep_index(jS + tid, gauge_axis)] = ys[tid];
    }
    if (s == 0 && tid < 7) dxi_full[tid < 6 ? 3 + tid : 12 + gauge_axis] = 0.0;  // the removed (gauge) parameters
    if (s > 0) flow_post(bar, (unsigned)(S - s));
    return;
  }
  // ================= bulk: at step s, columns left of block s, rows of block s+1
  const bool act = tid < 256;
  double *red = part;
  const int cj = tid & 31, ch = tid >> 5, nbulk = G - S;
  for (int s = S - 1; s >= 0; --s) {
    const int jS = s * SBW, jE = min(jS + SBW, D), jE2 = min(jE + SBW, D), np = jE2 - jE, ngrp = (jS + 31) / 32;
    // x_{s+1} -> the groups this workgroup owns, the rightmost (the next chain's) first
    if (np <= 0 || bid - S >= ngrp) continue;  // (uniform; owned groups only become fewer as s falls)
    if (tid == 0) flow_wait<8>(bar, (unsigned)(S - 1 - s), flag, max_polls);  // (the bulk has a chain step of slack: polls at leisure)
    __syncthreads();
    if (np > 0)
      for (int g0 = bid - S; g0 < ngrp; g0 += nbulk) {
        const int g = (bid - S) + ((ngrp - 1 - (bid - S)) / nbulk) * nbulk - (g0 - (bid - S));
        const int c = 32 * g + cj;
        double lv[16], xv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int r = 16 * ch + u;
          const bool ok = act && c < jS && r < np;
          lv[u] = ok ? M[(size_t)(jE + r) * ld + c] : 0.0;
          xv[u] = ok ? flow_load(y + jE + r) : 0.0;
        }
        const double yc = (tid < 32 && c < jS) ? flow_load(y + c) : 0.0;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int u = 0; u < 16; u += 2) {
          s0 += lv[u] * xv[u];
          s1 += lv[u + 1] * xv[u + 1];
        }
        if (act) red[ch * 32 + cj] = s0 + s1;
        __syncthreads();
        if (tid < 32 && c < jS) {
          double tot = 0.0;
#pragma unroll
          for (int k = 0; k < 8; ++k) tot += red[k * 32 + cj];
          flow_store(y + c, yc - tot);
        }
        flow_post(bar + 1 + g, (unsigned)(S - 1 - s));
        __syncthreads();
      }
  }
}

// ---- fallback: LU with partial pivoting (what np.linalg.solve / LAPACK gesv does, ref :146) ----
// Only reached when the Cholesky meets a non-positive pivot (reduced system not positive definite,
// e.g. a negative damping factor): rare, but a library path, so it is blocked and runs on the whole chip.
// Right-looking, panels of LU_NB columns, on the AUGMENTED matrix [F | rhs] (ld = D + 1: the row
// swaps, the triangular solve and the trailing update carry the forward substitution along):
//   k_lu_panel  one workgroup: partial pivoting inside the panel (rows swapped in the panel only)
//   k_lu_swap   the panel's row swaps on every other column
//   k_lu_trsm   U12 = L11^-1 A12 (a thread per column)
//   k_lu_gemm   A22 -= L21 U12 (64 x 64 tiles, K = LU_NB through LDS)
// then k_lu_backsub solves U x = y row by row.
constexpr int LU_NB = 32;

__global__ void k_compact_full(int D, int m, int gauge_axis, const double *__restrict__ Apk,
                               const double *__restrict__ bfull, double *__restrict__ F) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;  // j in [0, D]: column D is the right-hand side
  if (j > D) return;
  const int gi = keep_index(i, gauge_axis);
  if (j == D) { F[(size_t)i * (D + 1) + D] = bfull[gi]; return; }
  const int gj = keep_index(j, gauge_axis);
  F[(size_t)i * (D + 1) + j] = packed_sym(Apk, m, gi, gj);
}

__global__ __launch_bounds__(1024) void k_lu_panel(double *__restrict__ F, int D, int j0, int nb, int *__restrict__ ipiv,
                                                   int *__restrict__ flag) {
  __shared__ double s_val[1024];
  __shared__ int s_idx[1024];
  __shared__ int s_piv;
  const int tid = threadIdx.x, nt = blockDim.x, ld = D + 1;
  for (int c = 0; c < nb; ++c) {
    const int col = j0 + c;
    double best = -1.0;
    int bi = col;
    for (int i = col + tid; i < D; i += nt) {
      const double v = fabs(F[(size_t)i * ld + col]);
      if (v > best) { best = v; bi = i; }
    }
    s_val[tid] = best; s_idx[tid] = bi;
    __syncthreads();
    for (int off = nt >> 1; off > 0; off >>= 1) {
      if (tid < off && (s_val[tid + off] > s_val[tid] || (s_val[tid + off] == s_val[tid] && s_idx[tid + off] < s_idx[tid]))) {
        s_val[tid] = s_val[tid + off]; s_idx[tid] = s_idx[tid + off];
      }
      __syncthreads();
    }
    if (tid == 0) {
      s_piv = s_idx[0];
      ipiv[col] = s_idx[0];
      if (!(s_val[0] > 0.0)) atomicOr(flag, FLAG_LU_SINGULAR);  // exactly singular: LAPACK's info > 0 -> LinAlgError
    }
    __syncthreads();
    const int p = s_piv;
    if (p != col && tid < nb) {  // swap inside the panel (k_lu_swap does the other columns)
      const double a = F[(size_t)col * ld + j0 + tid];
      F[(size_t)col * ld + j0 + tid] = F[(size_t)p * ld + j0 + tid];
      F[(size_t)p * ld + j0 + tid] = a;
    }
    __syncthreads();
    const double ipv = 1.0 / F[(size_t)col * ld + col];
    const int rem = nb - c - 1;  // panel columns right of this one
    // multipliers and the rank-1 update of the rest of the panel, one row per (rem + 1) consecutive threads' work
    for (long long q = tid; q < (long long)(D - col - 1) * (rem + 1); q += nt) {
      const int i = col + 1 + (int)(q / (rem + 1)), cc = (int)(q % (rem + 1));
      const double mult = F[(size_t)i * ld + col] * ipv;
      if (cc == 0) ;  // (the multiplier itself is stored after the update below: other threads of the row still read the old value)
      else F[(size_t)i * ld + col + cc] -= mult * F[(size_t)col * ld + col + cc];
    }
    __syncthreads();
    for (int i = col + 1 + tid; i < D; i += nt) F[(size_t)i * ld + col] *= ipv;
    __syncthreads();
  }
}

__global__ void k_lu_swap(double *__restrict__ F, int D, int j0, int nb, const int *__restrict__ ipiv) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;  // every column of [F | rhs] outside the panel
  if (j >= j0) j += nb;
  if (j > D) return;
  const int ld = D + 1;
  for (int c = 0; c < nb; ++c) {
    const int r = j0 + c, p = ipiv[r];
    if (p != r) {
      const double a = F[(size_t)r * ld + j];
      F[(size_t)r * ld + j] = F[(size_t)p * ld + j];
      F[(size_t)p * ld + j] = a;
    }
  }
}

__global__ __launch_bounds__(256) void k_lu_trsm(double *__restrict__ F, int D, int j0, int nb) {
  __shared__ double L[LU_NB][LU_NB + 1];
  const int ld = D + 1;
  for (int e = threadIdx.x; e < nb * nb; e += blockDim.x) L[e / nb][e % nb] = F[(size_t)(j0 + e / nb) * ld + j0 + e % nb];
  __syncthreads();
  const int j = j0 + nb + blockIdx.x * blockDim.x + threadIdx.x;
  if (j > D) return;
  double u[LU_NB];
  for (int c = 0; c < nb; ++c) {
    double v = F[(size_t)(j0 + c) * ld + j];
    for (int cc = 0; cc < c; ++cc) v -= L[c][cc] * u[cc];
    u[c] = v;
    F[(size_t)(j0 + c) * ld + j] = v;
  }
}

__global__ __launch_bounds__(256) void k_lu_gemm(double *__restrict__ F, int D, int j0, int nb) {
  __shared__ double sL[64][LU_NB + 1], sU[LU_NB][65];
  const int ld = D + 1, i0 = j0 + nb + blockIdx.y * 64, c0 = j0 + nb + blockIdx.x * 64;
  for (int e = threadIdx.x; e < 64 * nb; e += 256) {
    const int r = e / nb, k = e % nb;
    sL[r][k] = (i0 + r < D) ? F[(size_t)(i0 + r) * ld + j0 + k] : 0.0;
  }
  for (int e = threadIdx.x; e < nb * 64; e += 256) {
    const int k = e >> 6, c = e & 63;
    sU[k][c] = (c0 + c <= D) ? F[(size_t)(j0 + k) * ld + c0 + c] : 0.0;
  }
  __syncthreads();
  const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
  double acc[4][4] = {};
  for (int k = 0; k < nb; ++k) {
    double a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = sL[tr + 16 * u][k];
#pragma unroll
    for (int v = 0; v < 4; ++v) b[v] = sU[k][tc + 16 * v];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u][v] += a[u] * b[v];
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = i0 + tr + 16 * u, c = c0 + tc + 16 * v;
      if (i < D && c <= D) F[(size_t)i * ld + c] -= acc[u][v];
    }
}

// U x = y (y = column D of the factored augmented matrix), row by row from the bottom; then the gauge slots
__global__ __launch_bounds__(1024) void k_lu_backsub(double *__restrict__ F, int D, int m, int gauge_axis,
                                                     double *__restrict__ dxi_full) {
  __shared__ double s_red[16];
  const int tid = threadIdx.x, nt = blockDim.x, ld = D + 1;
  for (int k = D - 1; k >= 0; --k) {
    double part = 0.0;
    for (int j = k + 1 + tid; j < D; j += nt) part += F[(size_t)k * ld + j] * F[(size_t)j * ld + D];
    const double t = block_sum(part, s_red);
    if (tid == 0) F[(size_t)k * ld + D] = (F[(size_t)k * ld + D] - t) / F[(size_t)k * ld + k];
    __syncthreads();
  }
  for (int i = tid; i < 9 * m; i += nt) dxi_full[i] = 0.0;
  __syncthreads();
  for (int i = tid; i < D; i += nt) dxi_full[keep_index(i, gauge_axis)] = F[(size_t)i * ld + D];
}
