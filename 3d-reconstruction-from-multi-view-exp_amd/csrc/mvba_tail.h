// The tail of an LM step (K5, K6) and the small state kernels -- gfx950: k_update_cams (trial cameras), k_backsub (dX, trial
// points), k_cam_tables (camera tables in device memory beyond LDS_CAMERAS), k_cost, k_residuals, k_sum_partials, k_project_obs
// (mvba_project) and k_similarity (mvba_apply_similarity).
//
// Included by mvba.hip inside its device-code namespace, after mvba_solve.h: uses block_sum, stage_cams, cam_row, dxi_row and PBS
// of mvba_device.h (the robust forms take its LossArgs), and obs_backsub, obs_cost, obs_resid, expand_cam and loss_rho of mvba_common.h.  Host launches
// (launch_tail_and_cost, launch_cost, cam_tables, mvba_residuals, mvba_project, mvba_apply_similarity) are in mvba.hip.

// ------------------------------------------------------------------ K6a: trial cameras (ref :263-281, utils.py:10-29)
__global__ void k_update_cams(int m, const double *__restrict__ cam15, const double *__restrict__ dxi,
                              double *__restrict__ out15) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const double *in = cam15 + (size_t)k * CAM_IN, *d = dxi + 9 * (size_t)k;
  double *o = out15 + (size_t)k * CAM_IN;
#pragma unroll
  for (int i = 0; i < 6; ++i) o[i] = in[i] + d[i];
  const double w0 = d[6], w1 = d[7], w2 = d[8];
  if (w0 == 0.0 && w1 == 0.0 && w2 == 0.0) {  // exact-zero shortcut (utils.py:14-15)
#pragma unroll
    for (int i = 0; i < 9; ++i) o[6 + i] = in[6 + i];
    return;
  }
  const double th = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  const double n0 = w0 / th, n1 = w1 / th, n2 = w2 / th;
  const double cs = cos(th), sn = sin(th), oc = 1.0 - cs;
  const double Q[9] = {oc * n0 * n0 + cs,      oc * n0 * n1 - sn * n2, oc * n0 * n2 + sn * n1,
                       oc * n1 * n0 + sn * n2, oc * n1 * n1 + cs,      oc * n1 * n2 - sn * n0,
                       oc * n2 * n0 - sn * n1, oc * n2 * n1 + sn * n0, oc * n2 * n2 + cs};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc)
      o[6 + 3 * r + cc] = Q[3 * r] * in[6 + cc] + Q[3 * r + 1] * in[9 + cc] + Q[3 * r + 2] * in[12 + cc];
}

// ------------------------------------------------------------------ K5
// dX_a = -E_a^-1 (sum_o F_ao dxi_k + dP_a), X' = X + dX  (ref :152, :260-261).  Eight lanes per
// point, one observation per lane.  y_o = 2 Jx^T (Jc dxi_k) is RECOMPUTED from the committed point
// and the committed camera (LDS table) instead of re-reading the 128-byte records: the kernel then
// moves 24 B/point + 4 B/observation instead of 128 B/observation (1.7 GB -> 0.25 GB at config 3),
// and it is evaluated as a directional derivative (obs_backsub: ~75 fp64 operations, the Jacobian rows
// are never formed) -- the same linear map the Schur kernel assembled, implied columns included.
// The trial cost is k_cost on the trial state (K6).
// BT threads per block: 256, or 1024 once the camera tables (m x 28 doubles) leave room for one block per CU only
// (beyond ~230 cameras: four waves per CU then; config 4's shard 0.47 -> see profiles/r04_m_*)
// ROBUST: F_ao of the weighted problem is w_o times the unweighted one: y_o is scaled by sqrt(w)^2 from `sqw`.
#define MVBA_BACKSUB_ARGS                                                                                                    \
  long long npts, int m, const long long *__restrict__ pt_ptr, const int *__restrict__ cam_idx, const double *__restrict__ PB, \
      const double *__restrict__ dxi, const double *__restrict__ X, const double *__restrict__ cam15, double f0,               \
      double *__restrict__ Xt, double *__restrict__ dX, const double *__restrict__ gcam, const double *__restrict__ gdxi
template <int G, int BT = 256, bool GCAM = false, bool ROBUST = false, typename... Robust>
__global__ __launch_bounds__(BT) void k_backsub(MVBA_BACKSUB_ARGS, Robust... robust) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *s_dxi = smem, *s_cam = smem + DXI_LDS * m;
  if constexpr (!GCAM)
    for (int i0 = threadIdx.x; i0 < 9 * m; i0 += 4 * blockDim.x) {  // (loads in batches of four: see k_point_inv)
      double t[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) t[u] = dxi[min(i0 + u * (int)blockDim.x, 9 * m - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * (int)blockDim.x;
        if (i < 9 * m) s_dxi[(i / 9) * DXI_LDS + i % 9] = t[u];
      }
    }
  stage_cams<GCAM>(cam15, m, f0, s_cam);  // (its barrier covers the update rows above as well)
  // G lanes per point (template).  Measured with 2 / 4 / 8 lanes: config 3 (10 observations per point)
  // 0.198 / 0.207 / 0.235 ms, config-4 shard (25 per point) 0.783 / 0.816 / 0.873 ms; one lane: 0.208
  const int s = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const long long a_first = (long long)blockIdx.x * (BT / G) + grp, a_step = (long long)gridDim.x * (BT / G);
  long long nx0 = 0, nx1 = 0;  // observation range of the NEXT point of this group, requested one iteration ahead
  if (a_first < npts) { nx0 = pt_ptr[a_first]; nx1 = pt_ptr[a_first + 1]; }
  for (long long a = a_first; a < npts; a += a_step) {
    const long long o0 = nx0, o1 = nx1;
    if (a + a_step < npts) { nx0 = pt_ptr[a + a_step]; nx1 = pt_ptr[a + a_step + 1]; }
    const double *pb = PB + PBS * a;
    const double pb0 = pb[0], pb1 = pb[1], pb2 = pb[2], pb3 = pb[3], pb4 = pb[4], pb5 = pb[5], pb6 = pb[6], pb7 = pb[7],
                 pb8 = pb[8];
    const double Xa0 = X[3 * a], Xa1 = X[3 * a + 1], Xa2 = X[3 * a + 2];
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    // (One observation's term of y stands twice below, batch and remainder, on purpose: as one function or lambda, in five
    // forms, the compiler contracted another product of the pb . y sums into its fma in 9 or 15 instantiations -- dX in the last bit.)
    // the camera ids of this lane's first PF observations in ONE batch (unconditional loads on clamped
    // indices: one memory latency per point instead of one per observation), the rare rest one by one
    constexpr int PF = 4;
    int kk[PF];
    double sw[PF];
    const long long olast = max(o1 - 1, o0);
#pragma unroll
    for (int u = 0; u < PF; ++u) kk[u] = cam_idx[min(o0 + s + G * u, olast)];
    if constexpr (ROBUST)
#pragma unroll
      for (int u = 0; u < PF; ++u) sw[u] = (robust, ...).sqw[min(o0 + s + G * u, olast)];
#pragma unroll
    for (int u = 0; u < PF; ++u)
      if (o0 + s + G * u < o1) {
        double t0, t1, t2;
        obs_backsub(Xa0, Xa1, Xa2, cam_row<GCAM>(gcam, s_cam, kk[u]), dxi_row<GCAM>(gdxi, s_dxi, kk[u]), f0, t0, t1, t2);
        if constexpr (ROBUST) {
          const double w = sw[u] * sw[u];
          t0 *= w;
          t1 *= w;
          t2 *= w;
        }
        y0 += t0;
        y1 += t1;
        y2 += t2;
      }
    for (long long o = o0 + s + G * PF; o < o1; o += G) {
      const int k = cam_idx[o];
      double t0, t1, t2;
      obs_backsub(Xa0, Xa1, Xa2, cam_row<GCAM>(gcam, s_cam, k), dxi_row<GCAM>(gdxi, s_dxi, k), f0, t0, t1, t2);
      if constexpr (ROBUST) {
        const double so = (robust, ...).sqw[o], w = so * so;
        t0 *= w;
        t1 *= w;
        t2 *= w;
      }
      y0 += t0;
      y1 += t1;
      y2 += t2;
    }
#pragma unroll
    for (int msk = 1; msk < G; msk <<= 1) {  // fixed butterfly: every lane ends with the group sum
      y0 += __shfl_xor(y0, msk, G);
      y1 += __shfl_xor(y1, msk, G);
      y2 += __shfl_xor(y2, msk, G);
    }
    if (s == 0) {
      const double d0 = -(pb0 * y0 + pb1 * y1 + pb2 * y2) - pb6;
      const double d1 = -(pb1 * y0 + pb3 * y1 + pb4 * y2) - pb7;
      const double d2 = -(pb2 * y0 + pb4 * y1 + pb5 * y2) - pb8;
      dX[3 * a] = d0; dX[3 * a + 1] = d1; dX[3 * a + 2] = d2;
      Xt[3 * a] = Xa0 + d0; Xt[3 * a + 1] = Xa1 + d1; Xt[3 * a + 2] = Xa2 + d2;
    }
  }
}

// Beyond LDS_CAMERAS: the expanded camera rows (and, for the back-substitution, the padded update rows) in device memory
__global__ void k_cam_tables(int m, const double *__restrict__ cam15, const double *__restrict__ dxi, double f0, double *__restrict__ cam18,
                             double *__restrict__ dxi10) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  expand_cam(cam15 + (size_t)k * CAM_IN, f0, cam18 + (size_t)k * CAM_LDS);
  if (dxi) {
    for (int i = 0; i < 9; ++i) dxi10[(size_t)k * DXI_LDS + i] = dxi[9 * (size_t)k + i];
    dxi10[(size_t)k * DXI_LDS + 9] = 0.0;
  }
}

// residual-only pass at a given state (initial cost, ref :85-87)
// LOSS: sum rho(|e|^2) instead, b = lb; same grid, same tree.
#define MVBA_COST_ARGS                                                                                                   \
  long long nobs, int m, const double *__restrict__ cam15, const double *__restrict__ X, const int *__restrict__ obs_pt, \
      const int *__restrict__ cam_idx, const double2 *__restrict__ xy, double f0, double *__restrict__ partials,        \
      const double *__restrict__ gcam
template <bool GCAM, int LOSS = LOSS_SQUARED, typename... Robust>
__global__ __launch_bounds__(512) void k_cost(MVBA_COST_ARGS, Robust... robust) {
  extern __shared__ __attribute__((aligned(16))) double s_cam[];
  __shared__ double s_red[16];
  stage_cams<GCAM>(cam15, m, f0, s_cam);
  double cost = 0.0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  // two dependent memory latencies per observation (its indices, then its point): the next
  // observation's indices are requested before this one is evaluated (clamped, unconditional loads)
  long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long olast = nobs - 1;
  int a_n = obs_pt[min(o, olast)], k_n = cam_idx[min(o, olast)];
  double2 z_n = xy[min(o, olast)];
  for (; o < nobs; o += stride) {
    const int a = a_n, k = k_n;
    const double2 z = z_n;
    const double X0 = X[3 * (size_t)a], X1 = X[3 * (size_t)a + 1], X2 = X[3 * (size_t)a + 2];
    const long long on = min(o + stride, olast);
    a_n = obs_pt[on];
    k_n = cam_idx[on];
    z_n = xy[on];
    const double so = obs_cost(X0, X1, X2, cam_row<GCAM>(gcam, s_cam, k), z.x, z.y, f0);
    if constexpr (LOSS != LOSS_SQUARED) cost += loss_rho<LOSS>(so, (robust, ...).b);
    else cost += so;
  }
  const double t = block_sum(cost, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// f0 e_o -- the residual in image units -- of every observation at a given state (mvba_residuals)
template <bool GCAM>
__global__ __launch_bounds__(256) void k_residuals(long long nobs, int m, const double *__restrict__ cam15, const double *__restrict__ X,
                                                   const int *__restrict__ obs_pt, const int *__restrict__ cam_idx,
                                                   const double2 *__restrict__ xy, double f0, double2 *__restrict__ out,
                                                   const double *__restrict__ gcam) {
  extern __shared__ __attribute__((aligned(16))) double s_cam[];
  stage_cams<GCAM>(cam15, m, f0, s_cam);
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < nobs; o += (long long)gridDim.x * blockDim.x) {
    const int a = obs_pt[o], k = cam_idx[o];
    const double2 z = xy[o];
    double e0, e1;
    obs_resid(X[3 * (size_t)a], X[3 * (size_t)a + 1], X[3 * (size_t)a + 2], cam_row<GCAM>(gcam, s_cam, k), z.x, z.y, f0, e0, e1);
    out[o] = make_double2(f0 * e0, f0 * e1);
  }
}

// out[0] = cost; the status flags ride along in the next 8 bytes so that the host needs ONE
// 16-byte device-to-host copy per trial step.
// `mail` (may be null): the same two words once more in pinned HOST memory, then -- behind a system-scope fence -- the
// sequence number the host is spinning on: the cost reaches the LM loop without a copy kernel and without waking a
// thread that sleeps in hipStreamSynchronize (~35 us between the last kernel of a step and the first of the next).
__global__ __launch_bounds__(1024) void k_sum_partials(const double *__restrict__ partials, int n,
                                                       double *__restrict__ out, const int *__restrict__ flag,
                                                       double *mail, unsigned long long seq) {
  __shared__ double s_red[16];
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) v += partials[i];
  const double t = block_sum(v, s_red);
  if (threadIdx.x == 0) {
    const int fl = *flag;
    out[0] = t;
    reinterpret_cast<int *>(out + 1)[0] = fl;
    if (mail) {
      mail[0] = t;
      reinterpret_cast<int *>(mail + 1)[0] = fl;
      __threadfence_system();
      __hip_atomic_store(reinterpret_cast<unsigned long long *>(mail + 2), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ------------------------------------------------------------------ projection (scene side of BA)
// x_o = K_k [R_k^T | -R_k^T t_k] [X_a; 1], inhomogeneous (ref lib/camera.py:13-14 get_camera_matrix,
// :30-34 project_points, :74-81 calc_projected_points) for an observation list.  The 3x4 camera
// matrices are formed once per block in LDS in the reference's order of operations (K times the
// stacked [R^T, -R^T t]); one thread per observation, coalesced reads of the index arrays and a
// coalesced 16-byte store.  obs_pt == nullptr: dense grid, observation o = point * m + camera.
__global__ __launch_bounds__(256) void k_project_obs(long long nobs, int m, const double *__restrict__ X,
                                                     const double *__restrict__ K, const double *__restrict__ R,
                                                     const double *__restrict__ t, const int *__restrict__ obs_pt,
                                                     const int *__restrict__ cam_idx, double2 *__restrict__ xy) {
  extern __shared__ double sP[];  // [m][12]
  for (int k = threadIdx.x; k < m; k += blockDim.x) {
    const double *Kk = K + 9 * (size_t)k, *Rk = R + 9 * (size_t)k, *tk = t + 3 * (size_t)k;
    double Rt[3][4];
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) Rt[i][j] = Rk[3 * j + i];
      Rt[i][3] = -(Rt[i][0] * tk[0] + Rt[i][1] * tk[1] + Rt[i][2] * tk[2]);
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) sP[12 * k + 4 * i + j] = Kk[3 * i] * Rt[0][j] + Kk[3 * i + 1] * Rt[1][j] + Kk[3 * i + 2] * Rt[2][j];
  }
  __syncthreads();
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < nobs; o += stride) {
    const long long a = obs_pt ? obs_pt[o] : o / m;
    const int k = cam_idx ? cam_idx[o] : (int)(o - a * m);
    const double *Xa = X + 3 * a, *P = sP + 12 * k;
    const double p0 = Xa[0] * P[0] + Xa[1] * P[1] + Xa[2] * P[2] + P[3];
    const double p1 = Xa[0] * P[4] + Xa[1] * P[5] + Xa[2] * P[6] + P[7];
    const double p2 = Xa[0] * P[8] + Xa[1] * P[9] + Xa[2] * P[10] + P[11];
    xy[o] = make_double2(p0 / p2, p1 / p2);
  }
}

// ------------------------------------------------------------------ way back to the input frame (ref :242-258)
// X <- s X R0^T + t0, t <- s t R0^T + t0, R <- R0 R on the committed state, in place: what the
// reference's optimize() does on the host before it returns (:198-200), without moving 48 MB of
// points across PCIe and through NumPy temporaries (8.5 ms at config 3, a quarter of a 10-iteration
// optimize()).
__global__ __launch_bounds__(256) void k_similarity(long long npts, int m, double *__restrict__ X, double *__restrict__ cam15,
                                                    const double *__restrict__ T13) {
  const double *R0 = T13, *t0 = T13 + 9;
  const double s = T13[12];
  const long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (a < npts) {
    double *x = X + 3 * a;
    const double x0 = s * x[0], x1 = s * x[1], x2 = s * x[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = x0 * R0[3 * i] + x1 * R0[3 * i + 1] + x2 * R0[3 * i + 2] + t0[i];
  }
  if (a < m) {
    double *c = cam15 + (size_t)a * CAM_IN;
    const double p0 = s * c[3], p1 = s * c[4], p2 = s * c[5];
    double Rn[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) Rn[3 * i + j] = R0[3 * i] * c[6 + j] + R0[3 * i + 1] * c[9 + j] + R0[3 * i + 2] * c[12 + j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) c[3 + i] = p0 * R0[3 * i] + p1 * R0[3 * i + 1] + p2 * R0[3 * i + 2] + t0[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) c[6 + i] = Rn[i];
  }
}
