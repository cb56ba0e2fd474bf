// Marginal covariances at the BA solution (mvba_covariance) -- kernels, gfx950.
//
// Included by mvba.hip inside its device-code namespace, after the K4 kernels (mvba_solve.h): uses NB, SBW, strip_offset, keep_index,
// tri_tile, mvba_d4, REC and the Cholesky factor k_chol_super leaves behind.  Nothing here runs on the LM path.
//
// After K4's factorisation of the gauge-reduced S = L L^T (no back-substitution) the factor is spread over three places:
//   M (d_Ared)   rows below each 128-column super-block: L
//   Lblk         the in-block 32 x 32 tiles below the diagonal of every super-block
//   Ztiles       L_JJ^-T of every 32 x 32 diagonal tile (upper triangle)
// The inverse S^-1 = L^-T L^-1 is formed in three steps on the f64 matrix cores (v_mfma_f64_16x16x4f64, the operand
// layout of k_chol_trail32: A/B lane (li, lk) holds element [li][k], C/D lane holds row lk + 4 q, column li):
//   k_cov_assemble   L's in-block tiles into M, W_JJ = L_JJ^-1 over M's diagonal tiles
//   k_cov_trtri      one launch per tile column J, last first: W_IJ = -(sum_{J<K<=I} W_IK L_KJ) W_JJ for every I > J, in
//                    place (LAPACK's trtri order).  Column J of L is read from a panel that the previous launch stashed,
//                    so that a workgroup may overwrite its tile of column J while others still need L there
//   k_cov_lauum      Sigma_IJ = sum_{K>=J} W_KI^T W_KJ for I <= J, scattered straight into the camera-block table below
// Camera-block table (Sigma, d_cov_sig): block (k, l), k <= l, of the full 9m x 9m S^-1 (zeros at the gauge slots), row-major
// 9 x 9, at SIG_BS * (k m - k (k-1) / 2 + l - k) doubles: the packed upper block triangle of strip_offset, block-major, each
// block padded to 82 doubles (656 bytes = 41 quad-words) so that the point pass gathers a block with 16-byte loads.
// k_point_cov then forms, per point a (observations in CSR order, any count):
//   C_a = 2 [E_a^-1 + E_a^-1 (4 sum_{o,o'} Jx_o^T (Jc_o Sigma_{k_o k_o'} Jc_o'^T) Jx_o') E_a^-1]
// with the implied record columns (u, v) -> 1/f0, t -> -Jx.  No atomics on floating-point data: every sum has a fixed order.

constexpr int SIG_BS = 82;  // doubles per camera block of the covariance table (81 + one pad)

__host__ __device__ __forceinline__ size_t sig_block(int k, int l, int m) {
  return (size_t)SIG_BS * ((size_t)k * m - (size_t)k * (k - 1) / 2 + (size_t)(l - k));
}

// lower-triangular W (or L) element of M; zero above the diagonal and outside the D x D matrix (clamped address)
__device__ __forceinline__ double cov_ldw(const double *M, int ld, int D, int r, int c) {
  const double v = M[(size_t)min(r, D - 1) * ld + min(c, D - 1)];
  return (r < D && c <= r) ? v : 0.0;
}

// One workgroup per 32-column tile J: W_JJ = (Ztile_J)^T over M's diagonal tile (lower triangle), and the in-block tiles of L
// below it from Lblk.
__global__ __launch_bounds__(256) void k_cov_assemble(double *M, int ld, int D, const double *__restrict__ Ztiles,
                                                      const double *__restrict__ Lblk) {
  const int J = blockIdx.x, s = J / 4, q = J % 4, jS = SBW * s;
  for (int e = threadIdx.x; e < NB * NB; e += 256) {
    const int i = e >> 5, j = e & 31, r = NB * J + i;
    if (r < D && j <= i) M[(size_t)r * ld + NB * J + j] = Ztiles[(size_t)J * NB * NB + j * NB + i];
  }
  for (int rr = q + 1; rr < 4; ++rr)
    for (int e = threadIdx.x; e < NB * NB; e += 256) {
      const int i = e >> 5, j = e & 31, r = jS + NB * rr + i;
      if (r < D) M[(size_t)r * ld + NB * J + j] = Lblk[(size_t)s * SBW * SBW + (size_t)(NB * rr + i) * SBW + NB * q + j];
    }
}

// Tile column J of W = L^-1 (J <= nt - 2), in place.  Workgroups 0 .. nt-2-J: output tile I = J + 1 + blockIdx.x; the four
// waves take K = J+1+w, J+5+w, ... and their partial tiles are summed in a fixed order through LDS, then multiplied by W_JJ.
// L_KJ comes from `pin` ([D][32]: column tile J of L by global row).  The remaining nt - J workgroups (J >= 1) stash column
// tile J - 1 of L (rows >= 32 J) into `pout` for the next launch: nobody writes that column in this one.  Launched once with
// J = nt - 1 (no output tiles) to stash the first column.
__global__ __launch_bounds__(256) void k_cov_trtri(double *M, int ld, int D, int nt, int J, const double *__restrict__ pin,
                                                   double *__restrict__ pout) {
  __shared__ double part[4][NB][NB + 1];
  __shared__ double wjj[NB][NB + 1];
  const int nrow = nt - 1 - J, tid = threadIdx.x;
  if ((int)blockIdx.x >= nrow) {
    const int I = J + (int)blockIdx.x - nrow;
    for (int e = tid; e < NB * NB; e += 256) {
      const int r = NB * I + (e >> 5);
      if (r < D) pout[(size_t)r * NB + (e & 31)] = M[(size_t)r * ld + NB * (J - 1) + (e & 31)];
    }
    return;
  }
  const int I = J + 1 + (int)blockIdx.x;
  const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const mvba_d4 zero4 = {0.0, 0.0, 0.0, 0.0};
  mvba_d4 acc[2][2] = {{zero4, zero4}, {zero4, zero4}};
  for (int K = J + 1 + wave; K <= I; K += 4) {
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = 16 * g + 4 * lk + u, rk = NB * K + k;
        double a[2], b[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          a[h] = cov_ldw(M, ld, D, NB * I + 16 * h + li, rk);
          const double pv = pin[(size_t)min(rk, D - 1) * NB + 16 * h + li];
          b[h] = rk < D ? pv : 0.0;
        }
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
          for (int rj = 0; rj < 2; ++rj) acc[ri][rj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ri], b[rj], acc[ri][rj], 0, 0, 0);
      }
  }
#pragma unroll
  for (int ri = 0; ri < 2; ++ri)
#pragma unroll
    for (int rj = 0; rj < 2; ++rj)
#pragma unroll
      for (int q = 0; q < 4; ++q) part[wave][16 * ri + lk + 4 * q][16 * rj + li] = acc[ri][rj][q];
  for (int e = tid; e < NB * NB; e += 256) wjj[e >> 5][e & 31] = cov_ldw(M, ld, D, NB * J + (e >> 5), NB * J + (e & 31));
  __syncthreads();
  for (int e = tid; e < NB * NB; e += 256) {
    const int i = e >> 5, j = e & 31;
    part[0][i][j] = (part[0][i][j] + part[1][i][j]) + (part[2][i][j] + part[3][i][j]);
  }
  __syncthreads();
  // W_IJ = -T W_JJ: wave w owns the 16 x 16 sub-tile (w >> 1, w & 1)
  const int ri = wave >> 1, rj = wave & 1;
  mvba_d4 x = zero4;
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = 16 * g + 4 * lk + u;
      x = __builtin_amdgcn_mfma_f64_16x16x4f64(part[0][16 * ri + li][k], wjj[k][16 * rj + li], x, 0, 0, 0);
    }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = NB * I + 16 * ri + lk + 4 * q;
    if (r < D) M[(size_t)r * ld + NB * J + 16 * rj + li] = -x[q];
  }
}

// Sigma = W^T W on the upper tile triangle: one workgroup per tile (I <= J), K = J .. nt-1 split over the four waves as above.
// Every element (r1 <= r2 of the reduced system) is written once to block (k1, k2) of the table, and its mirror image once
// more inside a diagonal block (k1 == k2): each address has exactly one writer.  The gauge slots are zeroed beforehand.
__global__ __launch_bounds__(256) void k_cov_lauum(const double *__restrict__ M, int ld, int D, int nt, int m, int gauge_axis,
                                                   double *__restrict__ sig) {
  __shared__ double part[4][NB][NB + 1];
  const int t = blockIdx.x, tid = threadIdx.x;
  int J, I;
  tri_tile(t, J, I);
  const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const mvba_d4 zero4 = {0.0, 0.0, 0.0, 0.0};
  mvba_d4 acc[2][2] = {{zero4, zero4}, {zero4, zero4}};
  for (int K = J + wave; K < nt; K += 4) {
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rk = NB * K + 16 * g + 4 * lk + u;
        double a[2], b[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          a[h] = cov_ldw(M, ld, D, rk, NB * I + 16 * h + li);
          b[h] = cov_ldw(M, ld, D, rk, NB * J + 16 * h + li);
        }
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
          for (int rj = 0; rj < 2; ++rj) acc[ri][rj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ri], b[rj], acc[ri][rj], 0, 0, 0);
      }
  }
#pragma unroll
  for (int ri = 0; ri < 2; ++ri)
#pragma unroll
    for (int rj = 0; rj < 2; ++rj)
#pragma unroll
      for (int q = 0; q < 4; ++q) part[wave][16 * ri + lk + 4 * q][16 * rj + li] = acc[ri][rj][q];
  __syncthreads();
  for (int e = tid; e < NB * NB; e += 256) {
    const int i = e >> 5, j = e & 31, r1 = NB * I + i, r2 = NB * J + j;
    if (r1 >= D || r2 >= D || r1 > r2) continue;
    const double v = (part[0][i][j] + part[1][i][j]) + (part[2][i][j] + part[3][i][j]);
    const int g1 = keep_index(r1, gauge_axis), g2 = keep_index(r2, gauge_axis), k1 = g1 / 9, k2 = g2 / 9;
    const int a1 = g1 - 9 * k1, a2 = g2 - 9 * k2;
    double *blk = sig + sig_block(k1, k2, m);
    blk[9 * a1 + a2] = v;
    if (k1 == k2 && a1 != a2) blk[9 * a2 + a1] = v;
  }
}

// cam[k][9][9] = 2 Sigma_kk (the unit covariance of camera k)
__global__ __launch_bounds__(256) void k_cov_cam_diag(int m, const double *__restrict__ sig, double *__restrict__ cam) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= 81LL * m) return;
  const int k = (int)(e / 81), i = (int)(e - 81LL * k);
  cam[e] = 2.0 * sig[sig_block(k, k, m) + i];
}

// Point-major pass: G lanes per point, lane p of the group takes the unordered observation pairs (i <= j) p, p + G, ... of
// its point (pairs numbered j (j+1) / 2 + i), gathers the two records and the camera block Sigma_{k_i k_j}, and accumulates the
// symmetric part of Jx_i^T (Jc_i Sigma Jc_j^T) Jx_j (counted twice for i < j) in six registers; the group sums them with a
// fixed butterfly and its first lane finishes C_a.  A point whose E_a has a Cholesky pivot below 1e-12 of its largest
// diagonal entry (e.g. a point seen once) sets FLAG_COV_POINT.
// Held points (mvba_set_point_hold): the instantiation with one trailing `const uint8_t *held` [N] gives a held point no pairs
// and no pivot test, and writes six zeros for it -- a point that is not an unknown has no covariance.
template <int G, typename... Held>
__global__ __launch_bounds__(256) void k_point_cov(long long N, int m, const long long *__restrict__ pt_ptr, const int *__restrict__ cam,
                                                   const double2 *__restrict__ rec, const double *__restrict__ PL,
                                                   const double *__restrict__ sig, double f0inv, double *__restrict__ out,
                                                   int *__restrict__ flag, Held... held) {
  static_assert(sizeof...(Held) <= 1, "at most the held mask");
  const int sub = threadIdx.x & (G - 1);
  const long long groups = (long long)gridDim.x * (256 / G);
  for (long long a = ((long long)blockIdx.x * 256 + threadIdx.x) / G; a < N; a += groups) {
    bool held_pt = false;  // (the same for the G lanes of a point)
    if constexpr (sizeof...(Held) == 1) held_pt = (held, ...)[a] != 0;
    const long long o0 = pt_ptr[a], d = pt_ptr[a + 1] - o0, npairs = held_pt ? 0 : d * (d + 1) / 2;
    double q6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long p = sub; p < npairs; p += G) {
      long long j = (long long)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
      while (j * (j + 1) / 2 > p) --j;
      while ((j + 1) * (j + 2) / 2 <= p) ++j;
      const long long i = p - j * (j + 1) / 2;
      const long long oi = o0 + i, oj = o0 + j;
      const int ki = cam[oi], kj = cam[oj];
      double2 ri[REC], rj[REC];
#pragma unroll
      for (int s = 0; s < REC; ++s) { ri[s] = rec[oi * REC + s]; rj[s] = rec[oj * REC + s]; }
      double sg[SIG_BS];
      {
        const mvba_quad *qs = reinterpret_cast<const mvba_quad *>(sig + sig_block(min(ki, kj), max(ki, kj), m));
#pragma unroll
        for (int s = 0; s < SIG_BS / 2; ++s) { const mvba_quad v = qs[s]; sg[2 * s] = v.x; sg[2 * s + 1] = v.y; }
      }
      // Jc rows (2 x 9) from a record: f | u, v | t = -Jx | omega
      double ci[2][9], cj[2][9];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        auto row = [&](const double2 *R, double (&c)[2][9]) {
          auto cmp = [&](const double2 v) { return r == 0 ? v.x : v.y; };
          c[r][0] = cmp(R[3]);
          c[r][1] = r == 0 ? f0inv : 0.0;
          c[r][2] = r == 1 ? f0inv : 0.0;
          c[r][3] = -cmp(R[0]); c[r][4] = -cmp(R[1]); c[r][5] = -cmp(R[2]);
          c[r][6] = cmp(R[4]); c[r][7] = cmp(R[5]); c[r][8] = cmp(R[6]);
        };
        row(ri, ci);
        row(rj, cj);
      }
      // (ki > kj cannot happen for ascending cam_idx; if it did, the stored block is Sigma_{kj ki} = Sigma_{ki kj}^T)
      const bool tr = ki > kj;
      double t2[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
      for (int r = 0; r < 9; ++r) {
        double u0 = 0.0, u1 = 0.0;  // (Sigma Jc_j^T)[r][0..1]
#pragma unroll
        for (int s = 0; s < 9; ++s) {
          const double v = tr ? sg[9 * s + r] : sg[9 * r + s];
          u0 += v * cj[0][s];
          u1 += v * cj[1][s];
        }
        t2[0][0] += ci[0][r] * u0; t2[0][1] += ci[0][r] * u1;
        t2[1][0] += ci[1][r] * u0; t2[1][1] += ci[1][r] * u1;
      }
      // X = Jx_i^T t Jx_j (3 x 3)
      double xi[2][3], xj[2][3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        xi[0][c] = ri[c].x; xi[1][c] = ri[c].y;
        xj[0][c] = rj[c].x; xj[1][c] = rj[c].y;
      }
      double X[3][3];
#pragma unroll
      for (int pp = 0; pp < 3; ++pp) {
        const double v0 = xi[0][pp] * t2[0][0] + xi[1][pp] * t2[1][0], v1 = xi[0][pp] * t2[0][1] + xi[1][pp] * t2[1][1];
#pragma unroll
        for (int qq = 0; qq < 3; ++qq) X[pp][qq] = v0 * xj[0][qq] + v1 * xj[1][qq];
      }
      const double w = (i == j) ? 0.5 : 1.0;  // X + X^T: both orders of an off-diagonal pair, the symmetric part of a diagonal one
      q6[0] += w * (X[0][0] + X[0][0]);
      q6[1] += w * (X[0][1] + X[1][0]);
      q6[2] += w * (X[0][2] + X[2][0]);
      q6[3] += w * (X[1][1] + X[1][1]);
      q6[4] += w * (X[1][2] + X[2][1]);
      q6[5] += w * (X[2][2] + X[2][2]);
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1)
#pragma unroll
      for (int c = 0; c < 6; ++c) q6[c] += __shfl_xor(q6[c], off, 64);
    if (sub == 0 && held_pt) {
      double *o = out + 6 * (size_t)a;
      o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = 0.0;
    } else if (sub == 0) {
      const double *pl = PL + 9 * (size_t)a;
      const double xx = pl[0], xy = pl[1], xz = pl[2], yy = pl[3], yz = pl[4], zz = pl[5];
      const double c00 = yy * zz - yz * yz, c01 = xz * yz - xy * zz, c02 = xy * yz - xz * yy;
      const double det = xx * c00 + xy * c01 + xz * c02;
      const double m2 = xx * yy - xy * xy;  // LDL^T pivots: xx, m2 / xx, det / m2
      const double big = fmax(xx, fmax(yy, zz)), tol = 1e-12 * big;
      const bool ok = isfinite(det) && xx > tol && m2 > tol * xx && det > tol * m2;
      if (!ok) atomicOr(flag, FLAG_COV_POINT);
      const double id = 1.0 / det;
      const double e[3][3] = {{c00 * id, c01 * id, c02 * id},
                              {c01 * id, (xx * zz - xz * xz) * id, (xy * xz - xx * yz) * id},
                              {c02 * id, (xy * xz - xx * yz) * id, (xx * yy - xy * xy) * id}};
      const double Q[3][3] = {{4.0 * q6[0], 4.0 * q6[1], 4.0 * q6[2]},
                              {4.0 * q6[1], 4.0 * q6[3], 4.0 * q6[4]},
                              {4.0 * q6[2], 4.0 * q6[4], 4.0 * q6[5]}};
      double Y[3][3];  // E^-1 Q
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Y[r][c] = e[r][0] * Q[0][c] + e[r][1] * Q[1][c] + e[r][2] * Q[2][c];
      auto z = [&](int r, int c) { return 2.0 * (e[r][c] + (Y[r][0] * e[0][c] + Y[r][1] * e[1][c] + Y[r][2] * e[2][c])); };
      double *o = out + 6 * (size_t)a;
      o[0] = z(0, 0); o[1] = z(0, 1); o[2] = z(0, 2); o[3] = z(1, 1); o[4] = z(1, 2); o[5] = z(2, 2);
    }
  }
}
