// mvba_covariance on the host, as stages: the entry point at the end is the table of contents, the stages above it stand in the
// order it calls them and each returns its status.  The order of launches, event records and copies on the stream is one
// sequence from cov_setup to cov_read_back; a rank of a sharded engine that could not set up still enters the all-reduce.
//
//   cov_setup         the four buffers (all or none), the events, the scratch of a mapped or compact engine
//   cov_linearize     the LM step's launches at c = 0 (K1, K3a, K3), or the NaN mark of a rank that could not set up
//   cov_reduce        the all-reduce of [A|b] and the sharded verdict
//   (launch_factor)   gauge strip + blocked Cholesky of the undamped S
//   cov_invert        W = L^-1 in place, Sigma = W^T W into the camera-block table, the mapped expansion
//   cov_blocks        the point pass and the camera blocks
//   cov_read_back     the status word, the four timings, the point and camera blocks
//   cov_expand_full   the table expanded on the host to cam_cov_full
//
// Included by mvba.hip after mvba_step.h: uses its launch_resid_jac, launch_point_inv, launch_schur, allreduce_Ab and launch_factor,
// mvba_engine.h's mvba_handle, cov_lanes of mvba_engine_host.h and the kernels of mvba_cov.h and mvba_map.h.
namespace {

// one call's arguments, sizes and events (ev[i] .. ev[i + 1] is timing i; destroyed with the call)
struct CovCall {
  mvba_handle *h;
  double *point_cov, *cam_cov, *cam_cov_full, *timings_ms;
  int D, ld, nt;
  int mv;        // a map's scratch table has mv camera blocks per side (mv <= m)
  size_t n_sig;  // doubles of the camera-block table
  hipEvent_t ev[5] = {};
  ~CovCall() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
};

// First call: the camera-block table, the trtri panels, the point and camera blocks -- all four or none (a failed
// allocation frees what it got, so that a later call never runs with some of them missing)
int cov_setup(CovCall &c) {
  mvba_handle *h = c.h;
  auto free_cov = [&]() {
    for (double **q : {&h->d_cov_sig, &h->d_cov_panel, &h->d_cov_pts, &h->d_cov_cam}) h->mem.release(*q);
  };
  int rc = MVBA_OK;
  if (!h->d_cov_sig || !h->d_cov_panel || !h->d_cov_pts || !h->d_cov_cam) {
    free_cov();
    rc = h->mem.alloc(&h->d_cov_sig, c.n_sig);
    if (!rc) rc = h->mem.alloc(&h->d_cov_panel, 2 * (size_t)h->D * NB);
    if (!rc) rc = h->mem.alloc(&h->d_cov_pts, 6 * (size_t)h->N);
    if (!rc) rc = h->mem.alloc(&h->d_cov_cam, 81 * (size_t)h->m);
    if (rc) free_cov();
  }
  for (auto &e : c.ev)
    if (!rc && hipEventCreate(&e) != hipSuccess) rc = fail(MVBA_ERR_HIP, "hipEventCreate failed");
  // With a parameter map k_cov_lauum scatters Sigma' (D' x D') through keep_index into a scratch table of mv camera blocks per side;
  // k_map_cov_expand then fills the real table with P Sigma' P^T.
  if (!rc && h->mapped && c.D > 0 && !h->d_cov_sigv) rc = h->mem.alloc(&h->d_cov_sigv, c.n_sig);
  // A compact engine: the point pass reads J_omega of both observations of a pair -- it gets full-layout records of its own, from a
  // second K1 launch below (the same E_a and dP_a once more), rather than a second layout of k_point_cov
  if (!rc && h->rec_compact && c.point_cov && h->nobs && !h->d_rec_full) rc = h->mem.alloc(&h->d_rec_full, (size_t)REC * h->nobs);
  return rc;
}

int cov_linearize(CovCall &c, int setup_rc) {
  mvba_handle *h = c.h;
  if (setup_rc) {
    // A rank that could not set up still takes part in the collective (the others would wait in it for ever): it marks
    // b[3] -- camera 0's t_x, a gauge slot the solve never reads -- with a NaN (all-ones bytes), so that every rank sees
    // it in the sum and fails the call with it.
    MVBA_HIP(hipMemsetAsync(h->d_b() + 3, 0xFF, sizeof(double), h->stream));
    return MVBA_OK;
  }
  MVBA_HIP(hipEventRecord(c.ev[0], h->stream));
  if (h->nobs && h->rec_compact && c.point_cov) launch_resid_jac(h, h->d_rec_full);
  if (h->nobs) launch_resid_jac(h);
  h->linearized = true; h->have_trial = false;
  launch_point_inv(h, 0.0);
  launch_schur(h, 0.0);
  MVBA_HIP(hipGetLastError());
  return MVBA_OK;
}

int cov_reduce(CovCall &c, int setup_rc, const std::string &setup_err) {
  mvba_handle *h = c.h;
  if (int rc = allreduce_Ab(h, false)) return rc;
  if (h->comm || h->host_ar) {
    double mark = 0.0;
    MVBA_HIP(hipMemcpyAsync(&mark, h->d_b() + 3, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MVBA_HIP(hipStreamSynchronize(h->stream));
    if (setup_rc) return fail(setup_rc, setup_err);
    if (std::isnan(mark))
      return fail(MVBA_ERR_HIP, "mvba_covariance: another rank could not allocate its covariance buffers (or the reduced system is not finite)");
  }
  return MVBA_OK;
}

// W = L^-1 in place in d_Ared, then Sigma = W^T W into the camera-block table (zeros at the gauge slots)
int cov_invert(CovCall &c) {
  mvba_handle *h = c.h;
  const int m = h->m, D = c.D, ld = c.ld, nt = c.nt;
  if (D > 0)
    hipLaunchKernelGGL(k_cov_assemble, dim3(nt), dim3(256), 0, h->stream, h->d_Ared, ld, D, (const double *)h->d_Ztiles,
                       (const double *)h->d_Lblk);
  double *panel[2] = {h->d_cov_panel, h->d_cov_panel + (size_t)D * NB};
  for (int J = nt - 1; J >= 0; --J) {
    const int grid = (nt - 1 - J) + (J >= 1 ? nt - J : 0);
    if (grid)
      hipLaunchKernelGGL(k_cov_trtri, dim3(grid), dim3(256), 0, h->stream, h->d_Ared, ld, D, nt, J, (const double *)panel[J & 1],
                         panel[(J + 1) & 1]);
  }
  MVBA_HIP(hipMemsetAsync(h->d_cov_sig, 0, sizeof(double) * c.n_sig, h->stream));
  if (h->mapped) {
    if (D > 0) {
      hipLaunchKernelGGL(k_cov_lauum, dim3(nt * (nt + 1) / 2), dim3(256), 0, h->stream, (const double *)h->d_Ared, ld, D, nt, c.mv,
                         h->gauge_axis, h->d_cov_sigv);
      hipLaunchKernelGGL(k_map_cov_expand, dim3((unsigned)((81 * m + 255) / 256), m), dim3(256), 0, h->stream, m, c.mv, h->gauge_axis,
                         (const int *)h->d_map_col, (const double *)h->d_cov_sigv, h->d_cov_sig);
    }
  } else
  hipLaunchKernelGGL(k_cov_lauum, dim3(nt * (nt + 1) / 2), dim3(256), 0, h->stream, (const double *)h->d_Ared, ld, D, nt, m,
                     h->gauge_axis, h->d_cov_sig);
  return MVBA_OK;
}

// k_point_cov at G lanes per point; `held`: nothing, or the mask (held points skip the pair loop and the pivot test: six zeros)
template <typename... M>
auto point_cov_kernel(int G) {
  return G == 64 ? k_point_cov<64, M...> : (G == 32 ? k_point_cov<32, M...> : (G == 16 ? k_point_cov<16, M...> : k_point_cov<8, M...>));
}

int cov_blocks(CovCall &c) {
  mvba_handle *h = c.h;
  const int m = h->m;
  if (h->N && c.point_cov) {
    const double deg = (double)h->nobs / (double)h->N;
    const int G = cov_lanes(0.5 * deg * (deg + 1.0));  // lanes per point by mean pair count
    const unsigned grid = (unsigned)std::min<long long>(8192, (h->N * G + 255) / 256);
    auto launch = [&](auto kern, auto... held) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, h->stream, h->N, m, (const long long *)h->d_pt_ptr, (const int *)h->d_cam,
                         (const double2 *)(h->rec_compact ? h->d_rec_full : h->d_rec), (const double *)h->d_PL, (const double *)h->d_cov_sig, 1.0 / h->f0, h->d_cov_pts,
                         h->d_flag, held...);
    };
    if (h->n_held) launch(point_cov_kernel<const uint8_t *>(G), (const uint8_t *)h->d_held);
    else launch(point_cov_kernel<>(G));
  }
  if (c.cam_cov)
    hipLaunchKernelGGL(k_cov_cam_diag, dim3((unsigned)((81LL * m + 255) / 256)), dim3(256), 0, h->stream, m,
                       (const double *)h->d_cov_sig, h->d_cov_cam);
  MVBA_HIP(hipGetLastError());
  return MVBA_OK;
}

int cov_read_back(CovCall &c) {
  mvba_handle *h = c.h;
  int fl = 0;
  MVBA_HIP(hipMemcpyAsync(&fl, h->d_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipStreamSynchronize(h->stream));
  if (fl) {
    MVBA_HIP(hipMemsetAsync(h->d_flag, 0, sizeof(int), h->stream));
    MVBA_HIP(hipStreamSynchronize(h->stream));
    if (fl & (FLAG_POINT_SINGULAR | FLAG_COV_POINT)) return fail(MVBA_ERR_SINGULAR, "Singular matrix (a point block E_a is singular: a point seen once, or without parallax)");
    return fail(MVBA_ERR_SINGULAR, "Singular matrix (the undamped reduced camera system is not positive definite)");
  }
  if (c.timings_ms)
    for (int i = 0; i < 4; ++i) {
      float ms = 0.f;
      MVBA_HIP(hipEventElapsedTime(&ms, c.ev[i], c.ev[i + 1]));
      c.timings_ms[i] = ms;
    }
  if (c.point_cov && h->N) MVBA_HIP(hipMemcpy(c.point_cov, h->d_cov_pts, sizeof(double) * 6 * h->N, hipMemcpyDeviceToHost));
  if (c.cam_cov) MVBA_HIP(hipMemcpy(c.cam_cov, h->d_cov_cam, sizeof(double) * 81 * h->m, hipMemcpyDeviceToHost));
  return MVBA_OK;
}

// the table, expanded on the host strip by strip (blocks (k, k..m-1) are contiguous): C = 2 S^-1, both triangles
int cov_expand_full(CovCall &c) {
  mvba_handle *h = c.h;
  const int m = h->m;
  const size_t n9 = h->n9();
  std::vector<double> strip((size_t)SIG_BS * m);
  for (int k = 0; k < m; ++k) {
    MVBA_HIP(hipMemcpy(strip.data(), h->d_cov_sig + sig_block(k, k, m), sizeof(double) * SIG_BS * (m - k), hipMemcpyDeviceToHost));
    for (int l = k; l < m; ++l) {
      const double *b = strip.data() + (size_t)SIG_BS * (l - k);
      for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) {
          const double v = 2.0 * b[9 * i + j];
          c.cam_cov_full[(9 * (size_t)k + i) * n9 + 9 * (size_t)l + j] = v;
          c.cam_cov_full[(9 * (size_t)l + j) * n9 + 9 * (size_t)k + i] = v;
        }
    }
  }
  return MVBA_OK;
}

}  // namespace

extern "C" int mvba_covariance(mvba_handle *h, double *point_cov, double *cam_cov, double *cam_cov_full, double *timings_ms) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  if (h->loss != LOSS_SQUARED)
    return fail(MVBA_ERR_BADARG, "mvba_covariance: the covariance is defined for the squared loss only (this engine has a robust loss)");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set");
  MVBA_HIP(hipSetDevice(h->device));
  const int D = h->solve_D();
  CovCall c{h, point_cov, cam_cov, cam_cov_full, timings_ms, D, h->solve_ld(), (D + NB - 1) / NB, (D + 6) / 9 + 1,
            sig_block(h->m, h->m, h->m)};  // (the block index of (m, m) is the block count)
  const int setup_rc = cov_setup(c);
  if (setup_rc && !(h->comm || h->host_ar)) return setup_rc;
  const std::string setup_err = setup_rc ? g_err : std::string();
  if (int rc = cov_linearize(c, setup_rc)) return rc;
  if (int rc = cov_reduce(c, setup_rc, setup_err)) return rc;
  MVBA_HIP(hipEventRecord(c.ev[1], h->stream));
  if (D > 0) launch_factor(h);
  MVBA_HIP(hipEventRecord(c.ev[2], h->stream));
  if (int rc = cov_invert(c)) return rc;
  MVBA_HIP(hipEventRecord(c.ev[3], h->stream));
  if (int rc = cov_blocks(c)) return rc;
  MVBA_HIP(hipEventRecord(c.ev[4], h->stream));
  if (int rc = cov_read_back(c)) return rc;
  return cam_cov_full ? cov_expand_full(c) : MVBA_OK;
}
