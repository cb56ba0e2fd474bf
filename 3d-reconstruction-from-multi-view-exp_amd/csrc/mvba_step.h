// The LM step on the host: mvba_linearize, mvba_try_step and mvba_commit, and the launches they are made of -- K1, K3a, K3 in the
// engine's form, the all-reduce of [A|b], K4 (factor, solve, the LU rescue, the mapped forms), the tail with the trial cost, and
// the device half of MVBA_CHECK_SOLVE.  mvba_try_step at the end reads as the step; mvba_covariance (mvba_cov_host.h) shares
// the launches up to the factor.
//
// Included by mvba.hip after the engine's small entry points: uses mvba_engine.h (mvba_handle with its [A|b] accessors, Timed,
// launch_loss and the kernel tables, cam_tables, launch_cost, global_cost), g_rccl of mvba_rccl.h, the width rules and
// reduced_system_residual of mvba_engine_host.h, and the kernels of the device headers.
namespace {
// The launches the LM step shares with mvba_covariance.  The callers put their own Timed scopes around them, so that the
// covariance does not add to the per-kernel statistics.
// `full_rec`: a compact engine's full-layout buffer for mvba_covariance's point pass (null: the engine's own records, in its layout)
void launch_resid_jac(mvba_handle *h, double2 *full_rec = nullptr) {  // K1 with K2 fused in, at the committed state
  const int kt = h->k1_threads;  // 8 waves share one camera table: 2 blocks = 16 waves per CU
  cam_tables(h, h->d_cam15[h->cur], nullptr);
  const int wpb = kt / 64;
  const int grid = std::max(1, std::min(2048 * 256 / kt, (h->n_tiles + wpb - 1) / wpb));
  if (h->rec_compact && !full_rec)  // (squared loss, camera table in LDS: mvba_create)
    hipLaunchKernelGGL((k_resid_jac<false, LOSS_SQUARED, CompactRec>), dim3(grid), dim3(kt), k1_lds_bytes(h->m, false, kt), h->stream, h->nobs, h->m,
                       h->d_cam15[h->cur], h->d_X[h->cur], h->d_obs_pt, h->d_cam, h->d_xy, h->f0, h->d_tiles, h->n_tiles, h->d_rec, h->d_PL,
                       h->d_tile_slot, h->d_PLsplit, h->d_cam18, CompactRec{h->d_res});
  else
  launch_loss(h, resid_jac_kernel(h->gcam, h->loss), dim3(grid), dim3(kt), k1_lds_bytes(h->m, h->gcam, kt), h->nobs, h->m, h->d_cam15[h->cur],
              h->d_X[h->cur], h->d_obs_pt, h->d_cam, h->d_xy, h->f0, h->d_tiles, h->n_tiles, full_rec ? full_rec : h->d_rec, h->d_PL,
              h->d_tile_slot, h->d_PLsplit, h->d_cam18);
  if (h->n_splits)
    hipLaunchKernelGGL(k_sum_split, dim3((9 * h->n_splits + 255) / 256), dim3(256), 0, h->stream, h->n_splits, h->d_splits,
                       h->d_PLsplit, h->d_PL);
}

void launch_point_inv(mvba_handle *h, double c) {  // K3a (also clears the packed [A|b] and the slot form's pacing counters)
  const long long nAb = (long long)h->n_Ab();
  const unsigned grid = (unsigned)std::max<long long>((h->N + 255) / 256, std::min<long long>((nAb + 1023) / 1024, 4096));
  const long long nprog = h->slot_w == LANES_W ? 0 : (long long)h->slot_nR * h->slot_nseg * PACE_STRIDE;
  const int want_r = h->schur_mode == SCHUR_DENSE ? 1 : 0;
  const double *Xc = h->rec_compact ? h->d_X[h->cur] : nullptr;  // a compact engine's point rows carry X_a (the state K1 linearised at)
  auto launch = [&](auto kern, auto... held) {
    hipLaunchKernelGGL(kern, dim3(std::max(grid, 1u)), dim3(256), 0, h->stream, h->N, c, h->d_PL, h->d_PB, h->d_flag, h->d_Ab, nAb, h->d_prog,
                       nprog, want_r, Xc, held...);
  };
  // held points (mvba_set_point_hold): the masked form; without a mask the launch is the one it always was
  if (h->n_held) launch(k_point_inv<const uint8_t *>, (const uint8_t *)h->d_held);
  else launch(k_point_inv<>);
}

void launch_schur(mvba_handle *h, double c) {  // K3 in the engine's form: [A|b] of this rank's points
  const int m = h->m;
  double *d_A = h->d_Ab, *d_b = h->d_b();
  if (h->use_pairs) {
    // 64-bit offsets only when the records or the point blocks (+ the padding row) span 4 GiB (MVBA_FORCE_BIG: at test sizes too)
    const bool big = (std::max<long long>(h->nobs, h->N) + 1) * 128LL >= (1LL << 32) || h->force_big;
    if (h->schur_mode == SCHUR_SLOTS && h->slot_w == LANES_W) {
      if (h->n_waves && h->rec_compact)
        hipLaunchKernelGGL(k_schur_lanes_compact, dim3(h->n_waves), dim3(64), LANES_LDS_C, h->stream, h->d_wdesc, h->d_wunits, h->d_it_x, h->d_rec,
                           h->d_PB, c, h->f0, h->d_partial, h->slot_nR, h->d_range_o0, h->d_res, h->d_units, h->d_cam15[h->cur]);
      else if (h->n_waves)
        hipLaunchKernelGGL(k_schur_lanes, dim3(h->n_waves), dim3(64), LANES_LDS, h->stream, h->d_wdesc, h->d_wunits, h->d_it_x, h->d_rec, h->d_PB, c,
                           h->f0, h->d_partial, h->slot_nR, h->d_range_o0);
    } else if (h->schur_mode == SCHUR_SLOTS) {
      if (h->n_waves)
        hipLaunchKernelGGL(k_schur_slots, dim3(h->n_waves), dim3(64), SLOT_LDS, h->stream, h->d_wdesc,
                           h->d_wunits, h->d_it_x, (const int *)nullptr, (const int *)nullptr, h->d_rec, h->d_PB, c, h->f0, h->d_partial,
                           h->slot_nR, h->d_seg_end, h->d_prog, h->slot_nseg, SLOT_LAG, h->d_range_o0);
    } else if (h->n_units) {  // (the robust kernels take sqrt(w) per observation as a plain trailing pointer)
      auto launch = [&](auto kern, auto... robust) {
        hipLaunchKernelGGL(kern, dim3(8 * h->q_max), dim3(64), PAIRS_LDS, h->stream, h->d_units, h->d_q_ptr, h->d_q_units, h->d_it_k, h->d_it_l,
                           h->d_it_a, h->d_rec, h->d_PB, c, h->f0, h->d_partial, robust...);
      };
      if (h->loss != LOSS_SQUARED) launch(big ? k_schur_pairs_big_robust : k_schur_pairs_robust, (const double *)h->d_sqw);
      else launch(big ? k_schur_pairs_big : k_schur_pairs);
    }
    hipLaunchKernelGGL(k_schur_reduce, dim3((unsigned)((long long)m * (m + 1) / 2)), dim3(128), 0, h->stream, m, h->d_unit_ptr,
                       h->d_partial, d_A, d_b);
  } else if (h->schur_mode == SCHUR_DENSE) {
    const int T = (9 * m + 15) / 16;
    launch_loss(h, dense_kernel(T, h->d_dense_obs != nullptr), dim3(h->dense_blocks), dim3(64 * (dense_consumers(T) + dense_ch(T))), dense_lds_bytes(T, m),
                (const double2 *)h->d_rec, (const double *)h->d_PB, (const int *)h->d_dense_obs, (long long)h->N, m, 1.0 / h->f0, h->d_dense_part);
    const long long n_el = (long long)h->n_Ab();
    hipLaunchKernelGGL(k_schur_dense_finish, dim3((unsigned)((n_el + 3) / 4)), dim3(256), 0, h->stream, m, T, h->dense_blocks,
                       (const double *)h->d_dense_part, c, d_A, d_b);
  }
}

int allreduce_Ab(mvba_handle *h, bool timed) {  // C1: [A|b] summed over the ranks (RCCL or the host transport)
  const size_t n = h->n_Ab();
  if (h->comm) {
    Timed t(h, timed ? MVBA_K_ALLREDUCE : -1);
    ncclResult_t r = g_rccl.AllReduce(h->d_Ab, h->d_Ab, n, ncclDouble, ncclSum, h->comm, h->stream);
    if (r != ncclSuccess) return fail(MVBA_ERR_RCCL, std::string("ncclAllReduce: ") + g_rccl.GetErrorString(r));
  } else if (h->host_ar) {  // host-staged transport: D2H, caller's sum, H2D (no RCCL; see mvba_comm_init_host)
    h->host_buf.resize(n);
    MVBA_HIP(hipMemcpyAsync(h->host_buf.data(), h->d_Ab, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    MVBA_HIP(hipStreamSynchronize(h->stream));
    const auto t0 = std::chrono::steady_clock::now();  // the wait above belongs to the Schur kernel, not to the exchange
    if (h->host_ar(h->host_ar_user, h->host_buf.data(), (int64_t)n)) return fail(MVBA_ERR_RCCL, "host all-reduce callback failed");
    MVBA_HIP(hipMemcpyAsync(h->d_Ab, h->host_buf.data(), sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    if (timed && h->profiling) {  // host wall time of the exchange (callback + staging copy issue); the device path uses events
      h->stats.ms[MVBA_K_ALLREDUCE] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      h->stats.launches[MVBA_K_ALLREDUCE] += 1;
    }
  }
  return MVBA_OK;
}

// tied x tied entries of the mapped system into M (row stride ld; mirror: both triangles of the LU rescue's full matrix)
void launch_map_tied(mvba_handle *h, double *M, int ld, int mirror) {
  if (!h->n_map_pairs) return;
  hipLaunchKernelGGL(k_map_tied, dim3(h->n_map_pairs, h->map_nblk), dim3(256), 0, h->stream, h->m, (const double *)h->d_Ab,
                     (const int *)h->d_map_ptr, (const int *)h->d_map_mem, (const int2 *)h->d_map_pairs, h->d_map_part);
  hipLaunchKernelGGL(k_map_tied_finish, dim3((h->n_map_pairs + 255) / 256), dim3(256), 0, h->stream, h->n_map_pairs, h->map_nblk, ld,
                     mirror, (const int2 *)h->d_map_pairs, (const double *)h->d_map_part, M);
}

void launch_factor(mvba_handle *h) {  // K4 without the back-substitution: gauge strip into d_Ared, blocked Cholesky of [A|b]
  const int m = h->m, D = h->solve_D();
  double *d_A = h->d_Ab, *d_b = h->d_b();
  const int ld = h->solve_ld();
  const int ntc = (D + NB - 1) / NB;
  if (h->mapped) {  // the mapped gather (mvba_map.h): the untied corner tile by tile, then the rows from the first tied unknown on
    const int U = h->map_U, ntu = (U + NB - 1) / NB;
    hipLaunchKernelGGL(k_map_compact, dim3(ntu * (ntu + 1) / 2 + (D + 255) / 256), dim3(256), 0, h->stream, D, ld, m, U, ntu, d_A, d_b,
                       h->d_map_ptr, h->d_map_mem, h->d_Ared, h->d_bar, 1 + 4 * ((D + SBW - 1) / SBW));
    if (U < D)
      hipLaunchKernelGGL(k_map_rows, dim3((D + 63) / 64, D - U), dim3(256), 0, h->stream, D, ld, m, U, d_A, h->d_map_ptr, h->d_map_mem,
                         h->d_Ared);
    launch_map_tied(h, h->d_Ared, ld, 0);
  } else
  hipLaunchKernelGGL(k_compact, dim3(ntc * (ntc + 1) / 2 + (D + 255) / 256), dim3(256), 0, h->stream, D, ld, m, h->gauge_axis, ntc, d_A, d_b,
                     h->d_Ared, h->d_bar, 1 + 4 * ((D + SBW - 1) / SBW));
  for (int jS = 0; jS < D; jS += SBW) {
    const int jE = std::min(jS + SBW, D);
    hipLaunchKernelGGL(k_chol_super, dim3((D + 1 - jE + 63) / 64), dim3(SUPER_THREADS), SUPER_LDS, h->stream, h->d_Ared, ld, D, jS,
                       h->d_Ztiles + (size_t)(jS / NB) * NB * NB, h->d_Lblk + (size_t)(jS / SBW) * SBW * SBW, h->d_flag);
    if (jE < D) {
      const int nt32 = (D + 1 - jE + NB - 1) / NB, nt64 = (D + 1 - jE + TB - 1) / TB;
      if (jE - jS == SBW && nt64 * (nt64 + 1) / 2 >= h->trail64_min)
        hipLaunchKernelGGL(k_chol_trail64, dim3(nt64 * (nt64 + 1) / 2), dim3(256), TRAIL64_LDS, h->stream, h->d_Ared, ld, D, jS, jE);
      else
        hipLaunchKernelGGL(k_chol_trail32, dim3(nt32 * (nt32 + 1) / 2), dim3(256), 0, h->stream, h->d_Ared, ld, D, jS, jE);
    }
  }
}
}  // namespace

extern "C" {

int mvba_linearize(mvba_handle *h) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set");
  MVBA_HIP(hipSetDevice(h->device));
  if (h->nobs) {
    Timed t(h, MVBA_K_RESID_JAC);  // K1 with K2 (per-point blocks) fused in
    launch_resid_jac(h);
  }
  MVBA_HIP(hipGetLastError());
  h->linearized = true; h->have_trial = false;
  h->stats.n_linearize++;
  return MVBA_OK;
}

}  // extern "C"

namespace {
// The pieces of the LM trial (mvba_try_step below reads as the step).
// With a parameter map the solve kernels run on the D' x D' mapped system and scatter x (through keep_index, as ever) into a
// scratch vector; k_map_expand then writes dxi = P x.  D' = 0 (everything held): dxi = 0, no solve.
double *solve_x(mvba_handle *h) { return h->mapped ? h->d_map_x : h->d_dxi; }
void launch_expand(mvba_handle *h) {
  const size_t n9 = h->n9();
  if (h->mapped && h->solve_D() > 0)
    hipLaunchKernelGGL(k_map_expand, dim3((unsigned)((n9 + 255) / 256)), dim3(256), 0, h->stream, (int)n9, h->gauge_axis, h->d_map_col,
                       h->d_map_x, h->d_dxi);
}

void launch_solve(mvba_handle *h, bool onepass) {  // K4: gauge strip, blocked Cholesky, back-substitution
  const int m = h->m, D = h->solve_D();
  double *d_x = solve_x(h);
  Timed t(h, MVBA_K_SOLVE);
  if (D == 0) {  // (only with a map)
    hipMemsetAsync(h->d_dxi, 0, sizeof(double) * h->n9(), h->stream);
    return;
  }
  launch_factor(h);
  const int ld = h->solve_ld();
  const int S = (D + SBW - 1) / SBW;
  if (onepass && (S == 1 || S < h->n_cu)) {  // one persistent pass for L^T x = y (see k_chol_backsolve_all)
    // (point to point, nobody pays for anybody else: one bulk workgroup per column group)
    const int ngrp = ((S - 1) * SBW + 31) / 32, nbulk = S > 1 ? std::max(1, std::min(h->n_cu - S, ngrp)) : 0;
    hipLaunchKernelGGL(k_chol_backsolve_all<true>, dim3(S + nbulk), dim3(SUPER_THREADS),
                       BACKSOLVE_LDS, h->stream, h->d_Ared, ld, D, m, h->gauge_axis, h->d_Ztiles, h->d_Lblk, d_x, h->d_flag,
                       h->d_bar, h->barrier_polls);
  } else
  for (int jS = ((D - 1) / SBW) * SBW; jS >= 0; jS -= SBW) {
    const int jE = std::min(jS + SBW, D), jE2 = std::min(jE + SBW, D);
    const int nwg = (jE == D) ? 1 : 1 + (jS + 255) / 256;
    hipLaunchKernelGGL(k_chol_backsolve, dim3(nwg), dim3(256), 0, h->stream, h->d_Ared, ld, D, m, h->gauge_axis, h->d_Ztiles,
                       h->d_Lblk + (size_t)(jS / SBW) * SBW * SBW, d_x, jS, jE, jE2);
  }
  launch_expand(h);
}

// The Cholesky met a non-positive pivot: the reduced system is not positive definite (e.g. a
// negative damping factor).  The reference's np.linalg.solve is LU with partial pivoting and
// does not care, so the solve is redone that way (slow path, rare).
int launch_lu_solve(mvba_handle *h) {
  const int m = h->m, D = h->solve_D();
  double *d_A = h->d_Ab, *d_b = h->d_b(), *d_x = solve_x(h);
  if (!h->d_lu) {
    int rc_ = h->mem.alloc(&h->d_lu, (size_t)h->D * (h->D + 1));  // (the default map's size: any map fits)
    if (rc_) return rc_;
    rc_ = h->mem.alloc(&h->d_ipiv, (size_t)h->D);
    if (rc_) return rc_;
  }
  MVBA_HIP(hipMemsetAsync(h->d_flag, 0, sizeof(int), h->stream));
  Timed t(h, MVBA_K_SOLVE);
  if (h->mapped) {
    hipLaunchKernelGGL(k_map_full, dim3((D + 1 + 255) / 256, D), dim3(256), 0, h->stream, D, m, d_A, d_b, h->d_map_ptr, h->d_map_mem, h->d_lu);
    launch_map_tied(h, h->d_lu, D + 1, 1);
  } else
  hipLaunchKernelGGL(k_compact_full, dim3((D + 1 + 255) / 256, D), dim3(256), 0, h->stream, D, m, h->gauge_axis, d_A, d_b, h->d_lu);
  for (int j0 = 0; j0 < D; j0 += LU_NB) {
    const int nb = std::min(LU_NB, D - j0), right = D + 1 - (j0 + nb);  // columns right of the panel incl. the rhs
    hipLaunchKernelGGL(k_lu_panel, dim3(1), dim3(1024), 0, h->stream, h->d_lu, D, j0, nb, h->d_ipiv, h->d_flag);
    hipLaunchKernelGGL(k_lu_swap, dim3((D + 1 - nb + 255) / 256), dim3(256), 0, h->stream, h->d_lu, D, j0, nb, h->d_ipiv);
    if (right > 0) hipLaunchKernelGGL(k_lu_trsm, dim3((right + 255) / 256), dim3(256), 0, h->stream, h->d_lu, D, j0, nb);
    const int below = D - (j0 + nb);
    if (below > 0)
      hipLaunchKernelGGL(k_lu_gemm, dim3((right + 63) / 64, (below + 63) / 64), dim3(256), 0, h->stream, h->d_lu, D, j0, nb);
  }
  hipLaunchKernelGGL(k_lu_backsub, dim3(1), dim3(1024), 0, h->stream, h->d_lu, D, m, h->gauge_axis, d_x);
  launch_expand(h);
  return MVBA_OK;
}

// K6a + K5/K6: trial cameras, back-substitution, trial cost -- and the cost read back (mailbox, or copy + sync)
int launch_tail_and_cost(mvba_handle *h, double *E_trial) {
  const int m = h->m, trial = 1 - h->cur;
  {
    Timed t(h, MVBA_K_BACKSUB_COST);
    hipLaunchKernelGGL(k_update_cams, dim3((m + 63) / 64), dim3(64), 0, h->stream, m, h->d_cam15[h->cur], h->d_dxi,
                       h->d_cam15[trial]);
    if (h->N) {
      const size_t lds = cam_lds_bytes(m, h->gcam, true);
      cam_tables(h, h->d_cam15[h->cur], h->d_dxi);
      // lanes per point by mean degree, threads per block by the camera table's size: the width rules of mvba_engine_host.h
      const int G = k5_lanes((double)h->nobs / (double)h->N), bt = table_block_threads(lds);
      const int nblk = (int)std::min<long long>(4096 * 256 / bt, (h->N * G + bt - 1) / bt);
      launch_loss(h, backsub_kernel(G, bt, h->gcam), dim3(nblk), dim3(bt), lds, h->N, m, h->d_pt_ptr, h->d_cam, h->d_PB, h->d_dxi,
                  h->d_X[h->cur], h->d_cam15[h->cur], h->f0, h->d_X[trial], h->d_dX, h->d_cam18, h->d_dxi10);
    }
    // K6: trial cost = the residual-only pass at the trial state (fixed grid, fixed tree: deterministic)
    int rc = launch_cost(h, h->d_cam15[trial], h->d_X[trial]);
    if (rc) return rc;
  }
  return global_cost(h, E_trial);
}

// Debug mode (MVBA_CHECK_SOLVE=1, read in mvba_create): the residual of the reduced system, b - A dxi over the kept parameters,
// from the packed [A|b] the solve started from (it is intact: k_compact copied it) and the dxi it produced -- on the host, in
// the plain loops of reduced_system_residual (mvba_engine_host.h).  The persistent back-substitution orders its hand-overs with sc1 accesses and explicit waits, not with the
// memory model's fences: a stale read there would be a silently wrong camera step, which this catches.
int check_solve_residual(mvba_handle *h) {
  std::vector<double> Ab(h->n_Ab()), x(h->n9());
  MVBA_HIP(hipMemcpyAsync(Ab.data(), h->d_Ab, sizeof(double) * Ab.size(), hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipMemcpyAsync(x.data(), h->d_dxi, sizeof(double) * x.size(), hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipStreamSynchronize(h->stream));
  const double worst = reduced_system_residual(Ab.data(), x.data(), h->m, h->gauge_axis, h->mapped ? h->map_ptr.data() : nullptr,
                                               h->mapped ? h->map_mem.data() : nullptr, h->solve_D());
  if (!(worst <= h->check_solve_tol))
    return fail(MVBA_ERR_STATE, "MVBA_CHECK_SOLVE: the dense solve left a relative residual of " + std::to_string(worst) +
                                    " on the reduced camera system (a stale hand-over in the back-substitution?)");
  return MVBA_OK;
}
}  // namespace

extern "C" {

int mvba_try_step(mvba_handle *h, double c, double *E_trial) {
  if (!h || !E_trial) return fail(MVBA_ERR_BADARG, "null argument");
  if (!h->linearized) return fail(MVBA_ERR_STATE, "try_step before linearize");
  MVBA_HIP(hipSetDevice(h->device));
  {
    Timed t(h, MVBA_K_POINT_INV);
    launch_point_inv(h, c);
  }
  if (h->use_pairs || h->schur_mode == SCHUR_DENSE) {
    Timed t(h, MVBA_K_SCHUR);
    launch_schur(h, c);
  }
  MVBA_HIP(hipGetLastError());
  int rc = allreduce_Ab(h, true);
  if (rc) return rc;
  launch_solve(h, h->chol_onepass);
  MVBA_HIP(hipGetLastError());
  h->stats.n_try_step++;
  rc = launch_tail_and_cost(h, E_trial);
  if (rc) return rc;
  if ((*h->h_flag & FLAG_WAIT_GAVE_UP) && !(*h->h_flag & FLAG_POINT_SINGULAR)) {
    // A wait of the persistent back-substitution gave up: its grid was not co-resident (another
    // process holds CUs -- e.g. ranks sharing a GPU).  Nothing is lost but time: the packed [A|b] is intact, so the
    // solve is redone with one launch per super-block (no waits), and this handle stays on that path.
    MVBA_HIP(hipMemsetAsync(h->d_flag, 0, sizeof(int), h->stream));
    h->chol_onepass = false;
    h->stats.n_barrier_fallback++;
    launch_solve(h, false);
    rc = launch_tail_and_cost(h, E_trial);
    if (rc) return rc;
  }
  if ((*h->h_flag & FLAG_NOT_POSDEF) && !(*h->h_flag & (FLAG_POINT_SINGULAR | FLAG_WAIT_GAVE_UP))) {  // not positive definite: LU with partial pivoting, and the tail again
    rc = launch_lu_solve(h);
    if (rc) return rc;
    h->stats.n_lu_fallback++;
    rc = launch_tail_and_cost(h, E_trial);
    if (rc) return rc;
  }
  if (*h->h_flag) {
    const int fl = *h->h_flag;
    hipMemsetAsync(h->d_flag, 0, sizeof(int), h->stream);
    if (fl & FLAG_WAIT_GAVE_UP) return fail(MVBA_ERR_HIP, "k_chol_backsolve_all: a wait for a progress word timed out twice (is another process holding the CUs?)");
    return fail(MVBA_ERR_SINGULAR, (fl & FLAG_POINT_SINGULAR) ? "Singular matrix" : "Singular matrix (reduced camera system)");
  }
  if (h->check_solve) {
    rc = check_solve_residual(h);
    if (rc) return rc;
  }
  h->have_trial = true;
  return MVBA_OK;
}

int mvba_commit(mvba_handle *h) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  if (!h->have_trial) return fail(MVBA_ERR_STATE, "commit without a trial step");
  h->cur = 1 - h->cur;
  h->have_trial = false; h->linearized = false;
  h->stats.n_commit++;
  return MVBA_OK;
}

}  // extern "C"
