// Linearisation (K1 with K2 fused in, K3a) -- kernels, gfx950: k_resid_jac (records, E_a, dP_a), k_sum_split (points of more
// than 64 observations), k_point_inv (damped inverses; clears [A|b] and the pacing counters).
//
// Included by mvba.hip inside its device-code namespace, after mvba_device.h: uses its stage_cams, cam_row, as_const, REC, PBS and
// LossArgs, and obs_math, ObsJ, loss_sqrt_w, wave_sync and the status bits of mvba_common.h.  Host launches (launch_resid_jac,
// launch_point_inv) are in mvba.hip.

// ------------------------------------------------------------------ K1
// One thread per observation, grid-stride over 256-observation tiles; camera table
// staged once per block.  Each wave transposes its 64 records through LDS so that
// every global store instruction writes 1 KiB contiguous (8 whole lines).
// K2 is fused in: the per-point blocks E_a = 2 sum Jx^T Jx (6 unique) and dP_a = 2 sum Jx^T e
// (ref :429-469, :519-556) are formed by a wave-level segmented sum over the (point-sorted)
// observations -- PL[a][9] = Exx,Exy,Exz,Eyy,Eyz,Ezz,dP0..2 -- so the records are not re-read.
// Algorithmic traffic: 24 B in + 128 B out per observation + (24 in + 72 out) B per point.
// LOSS: a robust loss scales the observation's Jacobian rows and residual by sqrt(w) before they are stored
// and summed -- the records, E_a and dP_a are then those of the weighted least-squares problem -- and writes sqrt(w) to `sqw`.
// COMPACT (a squared instantiation with one trailing CompactRec): the record is slots 0..3 -- 64 B, `rec` is
// [n_obs][REC_C] -- and the residual goes to CompactRec::res; a store instruction of the transpose still writes 1 KiB contiguous
// (16 records), the residuals of a wave are 1 KiB contiguous as they are.  104 B instead of 152 B per observation; E_a and dP_a
// are the same sums of the same values.
#define MVBA_RESID_JAC_ARGS                                                                                                 \
  long long nobs, int m, const double *__restrict__ cam15, const double *__restrict__ X, const int *__restrict__ obs_pt,   \
      const int *__restrict__ cam_idx, const double2 *__restrict__ xy, double f0, const int *__restrict__ tile_start,     \
      int n_tiles, double2 *__restrict__ rec, double *__restrict__ PL, const int *__restrict__ tile_slot,                 \
      double *__restrict__ PLsplit, const double *__restrict__ gcam
template <bool GCAM, int LOSS = LOSS_SQUARED, typename... Robust>
__global__ __launch_bounds__(1024, 4) void k_resid_jac(MVBA_RESID_JAC_ARGS, Robust... robust) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr bool COMPACT = is_compact_rec<Robust...>::value;
  static_assert(!COMPACT || LOSS == LOSS_SQUARED, "the compact record is the squared loss's");
  constexpr int RS = COMPACT ? REC_C : REC;  // slots of a record
  auto swz = [](int row) { return COMPACT ? (row >> 1) & 3 : row & 7; };
  double *s_cam = smem;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  // per-wave 8 KiB staging tile, 16-byte aligned behind the camera table
  double2 *stage = reinterpret_cast<double2 *>(smem + (GCAM ? 0 : ((m * CAM_LDS + 1) & ~1))) + wave * (64 * REC);
  // the same 8 KiB is reused for the per-point sums: contrib[9][CS] doubles (odd stride: the nine
  // components of one observation sit in nine different banks), then seg_start[65], pt[64]
  constexpr int CS = 65;
  double *contrib = reinterpret_cast<double *>(stage);
  int *seg_start = reinterpret_cast<int *>(contrib + 9 * CS), *seg_pt = seg_start + 66;
  stage_cams<GCAM>(cam15, m, f0, s_cam);
  // Wave tiles are POINT-ALIGNED (built once on the host): whole points packed greedily into at
  // most 64 observations, so every per-point sum below is complete inside one wave -> plain
  // stores, no atomics, bitwise-reproducible E_a / dP_a.  Only a point with more than 64
  // observations is split over tiles (tile_start < 0 marks such a tile: it holds ONE piece of ONE point, whose sums
  // go to slot tile_slot[tile] of a side buffer; k_sum_split adds a point's pieces in tile order afterwards).
  for (int tile = blockIdx.x * nwave + wave; tile < n_tiles; tile += gridDim.x * nwave) {
    const int ts0 = tile_start[tile], ts1 = tile_start[tile + 1];
    const bool split = ts0 < 0;
    const int slot = split ? as_const(tile_slot)[tile] : 0;  // (wave-uniform: a scalar load)
    const long long wbase = split ? ~ts0 : ts0;  // first observation of this wave's tile
    const int n = (int)((ts1 < 0 ? ~ts1 : ts1) - wbase);
    const long long o = wbase + lane;
    const bool live = lane < n;
    int a = -1;
    double c9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
      a = obs_pt[o];
      const int k = cam_idx[o];
      const double2 z = xy[o];
      const double *Xa = X + 3 * (size_t)a;
      ObsJ J;
      obs_math(Xa[0], Xa[1], Xa[2], cam_row<GCAM>(gcam, s_cam, k), z.x, z.y, f0, J);
      if constexpr (LOSS != LOSS_SQUARED) {
        const LossArgs la = (robust, ...);
        const double sw = loss_sqrt_w<LOSS>(J.e0 * J.e0 + J.e1 * J.e1, la.b);
        J.e0 *= sw;
        J.e1 *= sw;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
#pragma unroll
          for (int i = 0; i < 3; ++i) J.jx[rr][i] *= sw;
          J.jc[rr][0] *= sw;
#pragma unroll
          for (int i = 6; i < 9; ++i) J.jc[rr][i] *= sw;
        }
        la.sqw[o] = sw;
      }
      // swizzled slot position (s ^ swz(lane)): conflict-free ds_write_b128 (128-byte rows: lane & 7; 64-byte rows: eight
      // consecutive lanes cover the instruction's 128-byte bank window with (lane >> 1) & 3)
      double2 *row = stage + lane * RS;
      const int sw = swz(lane);
      row[0 ^ sw] = make_double2(J.jx[0][0], J.jx[1][0]);
      row[1 ^ sw] = make_double2(J.jx[0][1], J.jx[1][1]);
      row[2 ^ sw] = make_double2(J.jx[0][2], J.jx[1][2]);
      row[3 ^ sw] = make_double2(J.jc[0][0], J.jc[1][0]);
      if constexpr (COMPACT) {
        const CompactRec cr = (robust, ...);
        cr.res[o] = make_double2(J.e0, J.e1);  // (a wave's residuals: 1 KiB contiguous as they are)
      } else {
        row[4 ^ sw] = make_double2(J.jc[0][6], J.jc[1][6]);
        row[5 ^ sw] = make_double2(J.jc[0][7], J.jc[1][7]);
        row[6 ^ sw] = make_double2(J.jc[0][8], J.jc[1][8]);
        row[7 ^ sw] = make_double2(J.e0, J.e1);
      }
      // K2 fused: this observation's share of E_a = 2 sum Jx^T Jx and dP_a = 2 sum Jx^T e
      c9[0] = 2.0 * (J.jx[0][0] * J.jx[0][0] + J.jx[1][0] * J.jx[1][0]);
      c9[1] = 2.0 * (J.jx[0][0] * J.jx[0][1] + J.jx[1][0] * J.jx[1][1]);
      c9[2] = 2.0 * (J.jx[0][0] * J.jx[0][2] + J.jx[1][0] * J.jx[1][2]);
      c9[3] = 2.0 * (J.jx[0][1] * J.jx[0][1] + J.jx[1][1] * J.jx[1][1]);
      c9[4] = 2.0 * (J.jx[0][1] * J.jx[0][2] + J.jx[1][1] * J.jx[1][2]);
      c9[5] = 2.0 * (J.jx[0][2] * J.jx[0][2] + J.jx[1][2] * J.jx[1][2]);
      c9[6] = 2.0 * (J.jx[0][0] * J.e0 + J.jx[1][0] * J.e1);
      c9[7] = 2.0 * (J.jx[0][1] * J.e0 + J.jx[1][1] * J.e1);
      c9[8] = 2.0 * (J.jx[0][2] * J.e0 + J.jx[1][2] * J.e1);
    }
    wave_sync();  // wave-synchronous hand-over through LDS (in-order DS queue)
#pragma unroll
    for (int q = 0; q < RS; ++q) {
      const int ol = q * (64 / RS) + lane / RS, pos = lane % RS;  // local observation, stored position
      const double2 v = stage[ol * RS + pos];
      if (ol < n) rec[(wbase + ol) * RS + (pos ^ swz(ol))] = v;
    }
    wave_sync();
    // ---- per-point sums (wave-level segmented reduction; observations are sorted by point)
    const int a_prev = __shfl_up(a, 1, 64);
    const bool head = live && (lane == 0 || a != a_prev);
    const unsigned long long heads = __ballot(head);
    const int nseg = __popcll(heads);
#pragma unroll
    for (int q = 0; q < 9; ++q) contrib[q * CS + lane] = c9[q];
    if (head) {
      const int rank = __popcll(heads & ((1ull << lane) - 1ull));
      seg_start[rank] = lane;
      seg_pt[rank] = a;
    }
    if (lane == 0) seg_start[nseg] = n;
    wave_sync();
    const int sl = lane / 9, comp = lane - 9 * sl;
    for (int s0 = 0; s0 < nseg; s0 += 7) {
      const int sg = s0 + sl;
      if (sl < 7 && sg < nseg) {
        const int i0 = seg_start[sg], i1 = seg_start[sg + 1];
        double acc = 0.0;
        for (int i = i0; i < i1; ++i) acc += contrib[comp * CS + i];
        // (split: a piece of a > 64-observation point -> its slot of the side buffer; wave-uniform choice)
        if (split) PLsplit[9 * (size_t)slot + comp] = acc;
        else PL[9 * (size_t)seg_pt[sg] + comp] = acc;
      }
    }
    wave_sync();
  }
}

// The per-point blocks of points with more than 64 observations: their pieces in tile order (fixed order: no atomics).
__global__ void k_sum_split(int n_split, const int4 *__restrict__ splits /* point, first slot, pieces */,
                            const double *__restrict__ PLsplit, double *__restrict__ PL) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, sp = t / 9, comp = t - 9 * sp;
  if (sp >= n_split) return;
  const int4 d = splits[sp];
  double v = 0.0;
  for (int q = 0; q < d.z; ++q) v += PLsplit[9 * (size_t)(d.y + q) + comp];
  PL[9 * (size_t)d.x + comp] = v;
}

// ------------------------------------------------------------------ K3a
// PB[a][PBS] = inverse of E_a with diagonal*(1+c) (6 unique), v_a = E^-1 dP_a (3), pad: one
// 128-byte line per point, so a gather of the inverse touches one 64-byte sector.
// Also clears the packed [A|b] the Schur kernel is about to accumulate into (one launch less on
// the path; the grid is sized for whichever of the two jobs is larger).
// Held points (mvba_set_point_hold): the instantiation with one trailing `const uint8_t *held` [npts] writes the
// row of a point removed from the unknowns -- E^-1 = 0, v = 0, R = 0, the tenth double 1 (a point, sign code 0) -- and does not
// test that point's determinant.  Without a mask the engine launches k_point_inv<>, whose arguments and body are the kernel's
// as it was before there were masks.
// `Xc` (a compact-record engine, else null): the committed points; X_a goes into slots 6 and 7 of the row -- (X0, X1), (X2, 0) --
// which the dense form's R does not need there (want_r and Xc exclude each other).  Read as a ring, slots 6, 7, 0, 1, 2 are the
// ONE run k_schur_lanes_compact gathers for an off-diagonal item, 6, 7, 0 .. 4 for a diagonal one.  Held points get theirs too:
// their omega columns still enter c diag(G_k).
template <typename... Held>
__global__ __launch_bounds__(256) void k_point_inv(long long npts, double c, const double *__restrict__ PL,
                                                   double *__restrict__ PB, int *__restrict__ flag,
                                                   double *__restrict__ Ab, long long nAb, int *__restrict__ prog, long long nprog, int want_r,
                                                   const double *__restrict__ Xc, Held... held) {
  static_assert(sizeof...(Held) <= 1, "at most the held mask");
  // a block's 256 points are 18 KiB of PL and 32 KiB of PB, both contiguous: moved with coalesced
  // accesses through LDS (a thread reading its own 72-byte row / writing its own 128-byte line touches
  // 64 different lines per instruction)
  // (one buffer for both directions -- a thread takes its nine inputs into registers before anybody writes a result: 32 KiB per
  // block = four blocks per CU instead of three at 50 KiB)
  __shared__ double2 s_out[256 * 8];
  double *s_in = reinterpret_cast<double *>(s_out);
  const long long a0 = (long long)blockIdx.x * 256, a = a0 + threadIdx.x;
  for (long long i = a; i < nAb; i += (long long)gridDim.x * blockDim.x) Ab[i] = 0.0;
  for (long long i = a; i < nprog; i += (long long)gridDim.x * blockDim.x) prog[i] = 0;  // pacing counters of k_schur_slots
  if (a0 >= npts) return;  // (uniform)
  const int np = (int)min<long long>(256, npts - a0);
  {  // nine independent loads per thread, then their stores (one load and one store per trip waits for every load in turn)
    double t[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) t[i] = PL[9 * a0 + min((int)threadIdx.x + 256 * i, 9 * np - 1)];
#pragma unroll
    for (int i = 0; i < 9; ++i)
      if ((int)threadIdx.x + 256 * i < 9 * np) s_in[threadIdx.x + 256 * i] = t[i];
  }
  __syncthreads();
  double in[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) in[i] = s_in[9 * min((int)threadIdx.x, np - 1) + i];
  __syncthreads();
  bool free_pt = threadIdx.x < np;
  if constexpr (sizeof...(Held) == 1) {
    if (free_pt && (held, ...)[a] != 0) {  // (a < npts here)
      free_pt = false;
      double2 *out = s_out + 8 * threadIdx.x;
      const int sw = threadIdx.x & 7;
#pragma unroll
      for (int q = 0; q < 8; ++q) out[q ^ sw] = make_double2(0.0, q == 4 ? 1.0 : 0.0);
      if (Xc) {
        out[6 ^ sw] = make_double2(Xc[3 * a], Xc[3 * a + 1]);
        out[7 ^ sw] = make_double2(Xc[3 * a + 2], 0.0);
      }
    }
  }
  if (free_pt) {
    const double s = 1.0 + c;
    const double xx = in[0] * s, xy = in[1], xz = in[2], yy = in[3] * s, yz = in[4], zz = in[5] * s;
    const double c00 = yy * zz - yz * yz, c01 = xz * yz - xy * zz, c02 = xy * yz - xz * yy;
    const double det = xx * c00 + xy * c01 + xz * c02;
    if (!(det != 0.0) || !isfinite(det)) atomicOr(flag, FLAG_POINT_SINGULAR);  // singular 3x3 (ref :128 raises LinAlgError)
    const double id = 1.0 / det;
    const double i00 = c00 * id, i01 = c01 * id, i02 = c02 * id;
    const double i11 = (xx * zz - xz * xz) * id, i12 = (xy * xz - xx * yz) * id, i22 = (xx * yy - xy * xy) * id;
    const double g0 = in[6], g1 = in[7], g2 = in[8];
    // slot s of point p sits at s_out[8 p + (s ^ (p & 7))]: conflict-free 16-byte LDS stores, undone on the way out
    double2 *out = s_out + 8 * threadIdx.x;
    const int sw = threadIdx.x & 7;
    out[0 ^ sw] = make_double2(i00, i01);
    out[1 ^ sw] = make_double2(i02, i11);
    out[2 ^ sw] = make_double2(i12, i22);
    out[3 ^ sw] = make_double2(i00 * g0 + i01 * g1 + i02 * g2, i01 * g0 + i11 * g1 + i12 * g2);
    out[4 ^ sw] = make_double2(i02 * g0 + i12 * g1 + i22 * g2, 1.0);  // tenth double: 1 = a point (row N, the padding row, stays 0)
    if (want_r) {
      // the dense-visibility Schur form reads E^-1 = R S R^T from the row's last three slots: R lower triangular, S = diag(+-1) --
      // L D L^T with |D|^1/2 folded into the columns; S = I for the positive definite inverse of every LM step, but the damped
      // blocks of a NEGATIVE damping factor (the LU-path test; np.linalg.solve takes any system) are indefinite.  The signs ride in
      // the tenth double: 1 + (d0 < 0) + 2 (d1 < 0) + 4 (d2 < 0)  (nobody else reads it in this mode)
      const double d0 = i00, q0 = d0 != 0.0 ? 1.0 / d0 : 0.0, l10 = i01 * q0, l20 = i02 * q0;
      const double d1 = i11 - l10 * i01, q1 = d1 != 0.0 ? 1.0 / d1 : 0.0, l21 = (i12 - l20 * i01) * q1;
      const double d2 = i22 - l20 * i02 - l21 * l21 * d1;
      const double a0 = sqrt(fabs(d0)), a1 = sqrt(fabs(d1)), a2 = sqrt(fabs(d2));
      out[4 ^ sw].y = 1.0 + (d0 < 0.0 ? 1.0 : 0.0) + (d1 < 0.0 ? 2.0 : 0.0) + (d2 < 0.0 ? 4.0 : 0.0);
      out[5 ^ sw] = make_double2(a0, l10 * a0);
      out[6 ^ sw] = make_double2(l20 * a0, a1);
      out[7 ^ sw] = make_double2(l21 * a1, a2);
    } else {
      out[5 ^ sw] = out[6 ^ sw] = out[7 ^ sw] = make_double2(0.0, 0.0);
      if (Xc) {
        out[6 ^ sw] = make_double2(Xc[3 * a], Xc[3 * a + 1]);
        out[7 ^ sw] = make_double2(Xc[3 * a + 2], 0.0);
      }
    }
  }
  __syncthreads();
  double2 *dst = reinterpret_cast<double2 *>(PB + PBS * a0);
  for (int e = threadIdx.x; e < 8 * np; e += 256) {
    const int p = e >> 3, sl = e & 7;
    dst[e] = s_out[8 * p + (sl ^ (p & 7))];
  }
}
