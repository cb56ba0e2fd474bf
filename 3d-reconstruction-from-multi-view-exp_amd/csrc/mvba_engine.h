// The BA engine on the host: mvba_handle and what every entry point of the engine shares -- the event timers (Timed, drain_events,
// sync_and_drain), the cost mailbox (cost_mail, global_cost), the state read and write (read_state, write_state), the one launch
// path of squared and robust engines (LossKernel, launch_loss) with the four kernel tables, the LDS formulas, cam_tables and
// launch_cost, and the environment knobs of mvba_create (CreateKnobs).
//
// Included by mvba.hip after the device code and before mvba_create.h: uses DevBufs (mvba_host.h), the width rules and the cam15
// row of mvba_engine_host.h, g_rccl (mvba_rccl.h) and, of the device headers, the kernels the tables name with their constants.
// mvba_create.h, mvba_step.h, mvba_cov_host.h, mvba_debug.h and the start headers all work on this handle.
enum { SCHUR_PAIRS = 1, SCHUR_SLOTS = 2, SCHUR_DENSE = 3 };  // (0 was round 1's camera-strip form: the values are mvba_get_info's)
struct mvba_handle {
  // the device, the problem's sizes, the gauge
  int device = 0;
  hipStream_t stream = nullptr;
  DevBufs mem;  // every device buffer below (h->mem.alloc): freed by mvba_destroy, or early by h->mem.release
  long long N = 0, nobs = 0;
  int m = 0, gauge_axis = 0, D = 0, ld = 0;
  double f0 = 1.0;
  // topology, and K1's wave tiles over it
  long long *d_pt_ptr = nullptr;
  int *d_cam = nullptr, *d_obs_pt = nullptr;
  double2 *d_xy = nullptr;
  int *d_tiles = nullptr;  // K1 point-aligned wave tiles
  int *d_tile_slot = nullptr;      // points with more than 64 observations: slot of every piece tile in d_PLsplit,
  int4 *d_splits = nullptr;        // (point, first slot, pieces) per such point
  double *d_PLsplit = nullptr;
  int n_splits = 0;
  int n_tiles = 0;
  bool any_split = false;
  int k1_threads = 512;
  // camera tables in device memory
  bool gcam = false;                  // more than LDS_CAMERAS cameras: the kernels read the camera tables from device memory (d_cam18, d_dxi10)
  double *d_cam18 = nullptr, *d_dxi10 = nullptr;
  // K3's form, and the pair-major Schur index (k_schur_pairs): items sorted by (k, l, point), units, per-XCD work queues
  bool use_pairs = true;              // pair-major index present (schur_mode != SCHUR_DENSE)
  int schur_mode = 2;                 // SCHUR_PAIRS / SCHUR_SLOTS (see k_schur_slots) / SCHUR_DENSE
  bool index_on_device = false;       // the Schur index was built by the k_idx_* kernels (nothing to upload)
  bool force_big = false;             // MVBA_FORCE_BIG: the 64-bit-offset kernels at any size
  long long n_items = 0, n_items_offdiag = 0, n_slot_items = 0;
  int n_units = 0, q_max = 0;
  int *d_it_k = nullptr, *d_it_l = nullptr, *d_it_a = nullptr, *d_unit_ptr = nullptr, *d_q_ptr = nullptr, *d_q_units = nullptr;
  int4 *d_units = nullptr;
  double *d_partial = nullptr;
  // ... the slot form's waves over it
  int n_waves = 0, slot_nR = 8, slot_nseg = 0;
  int slot_w = PSTEP;                 // slot form: lists per wave = items per step (21: k_schur_slots, 64: k_schur_lanes, not paced)
  int lane_places = 0;                // lane form: waves of its kernel a CU holds, as the occupancy query answered when the ranges were counted
  long long *d_range_o0 = nullptr;    // slot form: first observation of every point range (the record base of its waves)
  int *d_seg_end = nullptr, *d_prog = nullptr;
  int4 *d_wdesc = nullptr;
  int *d_it_x = nullptr;              // slot form: the step-major index, 64 ints per step (k[21] | l[21] | a[21] | pad); lane form: 128 (w0[64] | w1[64])
  int *d_wunits = nullptr;
  // ... and the dense form, which has no index
  double *d_dense_part = nullptr;     // SCHUR_DENSE: partial tiles per workgroup
  int *d_dense_obs = nullptr;         // ... and, with missing observations, the observation of every (point, camera) or -1
  int dense_blocks = 0, dense_tiles = 0;
  // state: [cur] committed, [1-cur] trial; the transform of mvba_apply_similarity
  double *d_X[2] = {nullptr, nullptr}, *d_cam15[2] = {nullptr, nullptr};
  int cur = 0;
  bool have_params = false, linearized = false, have_trial = false;
  double *d_sim = nullptr;
  // linearisation
  double2 *d_rec = nullptr;  // [n_obs][8] double2: one 128-B line per observation
  // the compact record (decided by mvba_create: lane form, squared loss, camera table in LDS, not MVBA_REC=full):
  // d_rec is [n_obs + 1][REC_C] -- J_X and d/df --, the residuals are d_res [n_obs + 1], PB carries X_a; d_rec_full is the full-layout
  // buffer mvba_covariance re-linearises into for its point pass, allocated on its first call
  bool rec_compact = false;
  double2 *d_res = nullptr, *d_rec_full = nullptr;
  double *d_PL = nullptr, *d_PB = nullptr;
  // reduced system: [A (9m x 9m) | b (9m)] contiguous for the all-reduce (n_A(), n_Ab(), d_b() below), and K4's solve of it
  double *d_Ab = nullptr, *d_Ared = nullptr, *d_Ztiles = nullptr, *d_Lblk = nullptr, *d_dxi = nullptr, *d_dX = nullptr, *d_lu = nullptr;
  int *d_ipiv = nullptr;
  unsigned *d_bar = nullptr;
  int n_cu = 1;
  bool chol_onepass = true;  // L^T x = y as one persistent launch (MVBA_CHOL=launches: one launch per super-block)
  int trail64_min = 200;     // trailing updates of at least this many 64 x 64 workgroups run k_chol_trail64 (MVBA_TRAIL64_MIN)
  unsigned barrier_polls = 1u << 22;  // what a wait of that launch polls before it gives up (MVBA_CHOL_BARRIER_POLLS)
  bool check_solve = false;           // MVBA_CHECK_SOLVE=1: every accepted dense solve is checked on the host against the packed system it solved
  double check_solve_tol = 1e-8;      // (MVBA_CHECK_SOLVE=<t> with 0 < t < 1: that tolerance -- the tests ask for an impossible one to see the check fire)
  // cost and the status word
  double *d_partials = nullptr, *d_cost = nullptr, *h_cost = nullptr;
  double *d_mail = nullptr;               // device address of h_cost (pinned, mapped): the cost kernel's mailbox
  unsigned long long cost_seq = 0;
  bool mail_pending = false;
  int n_partials = 0, cost_grid = 0;
  int *d_flag = nullptr, *h_flag = nullptr;
  // comm
  ncclComm_t comm = nullptr;
  int rccl_version = 0;
  mvba_host_allreduce_fn host_ar = nullptr;  // host-staged transport (mvba_comm_init_host) instead of RCCL
  void *host_ar_user = nullptr;
  std::vector<double> host_buf;
  int rank = 0, nranks = 1;
  double *d_allcost = nullptr, *h_allcost = nullptr;
  // debug log (mvba_snapshot): committed states kept in device memory, SNAP_SLAB entries per allocation
  std::vector<double *> snap_slabs;
  long long n_snap = 0;
  // profiling
  int profiling = 0;  // 0 off, 1 every phase, 2 the Schur and residual-Jacobian kernels only (mvba_set_profiling)
  mvba_stats stats{};
  struct Ev { int kid; hipEvent_t a, b; };
  std::vector<Ev> pending;
  std::vector<hipEvent_t> pool;
  // covariances (mvba_covariance), allocated on the first call: the camera-block table of S^-1, the two column panels of the
  // triangular inverse, the point and camera blocks
  double *d_cov_sig = nullptr, *d_cov_panel = nullptr, *d_cov_pts = nullptr, *d_cov_cam = nullptr;
  // robust loss (mvba_create_robust), fixed for the engine's life: LOSS_* , b = (delta / f0)^2, and sqrt(w) of
  // every observation at the last linearisation (K1 writes it, K3 and K5 read it)
  int loss = LOSS_SQUARED;
  double loss_b = 0.0;
  double *d_sqw = nullptr;
  // buffers of single entry points, allocated on the first call
  double2 *d_resid = nullptr;  // mvba_residuals
  double *d_init_cams = nullptr;  // mvba_triangulate_state: the committed cameras as K, R, t ([m][9 + 9 + 3])
  // parameter map (mvba_set_parameter_map); mapped == false: the default map, none of this is touched.
  // n_free unknowns, the first map_U of them untied; col / CSR transpose on the device (allocated on the first map), the
  // scratch vector the back-substitution scatters x into, the scratch camera-block table of a mapped mvba_covariance
  bool mapped = false;
  int n_free = 0, map_ld = 0, map_U = 0;
  std::vector<int> map_col, map_ptr, map_mem;
  int *d_map_col = nullptr, *d_map_ptr = nullptr, *d_map_mem = nullptr;
  double *d_map_x = nullptr, *d_cov_sigv = nullptr;
  int2 *d_map_pairs = nullptr;  // the (i, j <= i) pairs of tied unknowns, n_map_pairs of them; map_nblk partial sums per pair
  double *d_map_part = nullptr;
  int n_map_pairs = 0, map_nblk = 1;
  // held points (mvba_set_point_hold): the mask as 0 / 1 bytes [N], allocated on the first mask with a held point;
  // n_held == 0: no mask, none of this is touched
  uint8_t *d_held = nullptr;
  long long n_held = 0;
  int solve_D() const { return mapped ? n_free : D; }     // order and row stride of the system K4 solves
  int solve_ld() const { return mapped ? map_ld : ld; }
  size_t n9() const { return 9 * (size_t)m; }             // the packed [A|b] in d_Ab: 9 m camera parameters, A's strips, then b
  size_t n_A() const { return strip_offset(m, m); }
  size_t n_Ab() const { return n_A() + n9(); }
  double *d_b() const { return d_Ab + n_A(); }
};

namespace {

const char *kKernelNames[MVBA_K_COUNT] = {"resid_jac", "point_blocks", "point_inv", "schur",
                                          "allreduce", "solve",        "backsub_cost", "cost"};

struct Timed {
  mvba_handle *h;
  int kid;
  hipEvent_t a = nullptr, b = nullptr;
  bool on = false;
  Timed(mvba_handle *h_, int kid_) : h(h_), kid(kid_) {
    // level 2: the two kernels a roofline is quoted for, nothing else (every timed phase is two marker packets on the
    // stream and ~10 us of a 2.5 ms step)
    on = kid >= 0 && (h->profiling == 1 || (h->profiling == 2 && (kid == MVBA_K_SCHUR || kid == MVBA_K_RESID_JAC)));  // (kid -1: never)
    if (!on) return;
    auto get = [&]() {
      hipEvent_t e;
      if (!h->pool.empty()) { e = h->pool.back(); h->pool.pop_back(); }
      else hipEventCreate(&e);
      return e;
    };
    a = get(); b = get();
    hipEventRecord(a, h->stream);
  }
  ~Timed() {
    if (!on) return;
    hipEventRecord(b, h->stream);
    h->pending.push_back({kid, a, b});
  }
};

void drain_events(mvba_handle *h) {  // call after a stream sync
  for (auto &p : h->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      h->stats.ms[p.kid] += ms;
      h->stats.launches[p.kid] += 1;
    }
    h->pool.push_back(p.a);
    h->pool.push_back(p.b);
  }
  h->pending.clear();
}

int sync_and_drain(mvba_handle *h) {
  MVBA_HIP(hipStreamSynchronize(h->stream));
  drain_events(h);
  return MVBA_OK;
}

// The state (points, cameras as cam15 rows) at a device address -- the committed one, or an entry of the debug log -- to the C
// interface's arrays, and into the committed state from host memory (mvba_set_params: waits, the arrays are the caller's) or from
// device memory (mvba_snapshot_restore: ordered on the stream, no host wait).  A new state voids linearisation and trial.
int read_state(mvba_handle *h, const double *src_X, const double *src_cam, double *X, double *f, double *u, double *t, double *R) {
  std::vector<double> cam((size_t)h->m * CAM_IN);
  MVBA_HIP(hipMemcpyAsync(X, src_X, sizeof(double) * 3 * h->N, hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipMemcpyAsync(cam.data(), src_cam, sizeof(double) * cam.size(), hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipStreamSynchronize(h->stream));
  unpack_cam15(cam.data(), h->m, f, u, t, R);
  return MVBA_OK;
}
int write_state(mvba_handle *h, const double *src_X, const double *src_cam, hipMemcpyKind kind) {
  MVBA_HIP(hipMemcpyAsync(h->d_X[h->cur], src_X, sizeof(double) * 3 * h->N, kind, h->stream));
  MVBA_HIP(hipMemcpyAsync(h->d_cam15[h->cur], src_cam, sizeof(double) * CAM_IN * h->m, kind, h->stream));
  if (kind == hipMemcpyHostToDevice) MVBA_HIP(hipStreamSynchronize(h->stream));
  h->have_params = true; h->linearized = false; h->have_trial = false;
  return MVBA_OK;
}

// Sum of the per-rank costs in rank order and the OR of the per-rank status flags: both identical on
// every rank, so that all ranks take the same accept/reject, LU-rescue and error decisions (a
// rank that branched alone would leave the others waiting in the next collective).  (C1b: one
// all-gather of 16 bytes per rank per trial, on top of C1.)
inline void cpu_relax() {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
  __builtin_ia32_pause();
#endif
}

// Single rank, not every phase timed: the cost kernel mails its result to pinned host memory (see k_sum_partials).
// Returns the device address of the mailbox and advances the sequence number, or null for the copy + sync path.
double *cost_mail(mvba_handle *h) {
  if (h->comm || h->host_ar || h->profiling == 1 || !h->d_mail) return nullptr;
  ++h->cost_seq;
  h->mail_pending = true;
  return h->d_mail;
}

int global_cost(mvba_handle *h, double *E) {
  if (h->mail_pending) {
    h->mail_pending = false;
    volatile unsigned long long *seq = reinterpret_cast<volatile unsigned long long *>(h->h_cost + 2);
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (unsigned spins = 0;; ++spins) {
      if (*seq == h->cost_seq) { seen = true; break; }
      // (everything earlier on the stream is complete once the number has arrived; if it does not arrive -- a fault, a
      // hung kernel -- the ordinary synchronisation below reports what happened)
      if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;
      cpu_relax();
    }
    if (seen) {
      std::atomic_thread_fence(std::memory_order_acquire);
      drain_events(h);  // (level 2: the timers of K1 and K3 ended before the cost kernel started)
      *E = h->h_cost[0];
      return MVBA_OK;
    }
    int rc = sync_and_drain(h);
    if (rc) return rc;
    *E = h->h_cost[0];
    return MVBA_OK;
  }
  if (h->comm) {
    Timed t(h, MVBA_K_ALLREDUCE);
    ncclResult_t r = g_rccl.AllGather(h->d_cost, h->d_allcost, 2, ncclDouble, h->comm, h->stream);
    if (r != ncclSuccess) return fail(MVBA_ERR_RCCL, std::string("ncclAllGather: ") + g_rccl.GetErrorString(r));
    MVBA_HIP(hipMemcpyAsync(h->h_allcost, h->d_allcost, 2 * sizeof(double) * h->nranks, hipMemcpyDeviceToHost, h->stream));
  } else {
    MVBA_HIP(hipMemcpyAsync(h->h_cost, h->d_cost, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));  // cost + flags
  }
  int rc = sync_and_drain(h);
  if (rc) return rc;
  if (h->host_ar) {  // all-gather as a sum of one-hot slices: {cost, flags as a count} per rank
    std::vector<double> v(2 * (size_t)h->nranks, 0.0);
    v[2 * h->rank] = h->h_cost[0];
    v[2 * h->rank + 1] = (double)*h->h_flag;  // small non-negative integer: exact in a double
    if (h->host_ar(h->host_ar_user, v.data(), (int64_t)v.size())) return fail(MVBA_ERR_RCCL, "host all-reduce callback failed");
    double s = 0.0;
    int fl = 0;
    for (int i = 0; i < h->nranks; ++i) { s += v[2 * i]; fl |= (int)v[2 * i + 1]; }
    *E = s;
    *h->h_flag = fl;
  } else if (h->comm) {
    double s = 0.0;
    int fl = 0;
    for (int i = 0; i < h->nranks; ++i) {
      s += h->h_allcost[2 * i];
      int f;
      memcpy(&f, &h->h_allcost[2 * i + 1], sizeof(int));
      fl |= f;
    }
    *E = s;
    *h->h_flag = fl;
  } else {
    *E = *h->h_cost;
  }
  return MVBA_OK;
}

// ---- one launch path for squared and robust engines.  A robust instantiation takes the arguments of the squared
// one and a trailing LossArgs; LossKernel holds the two, launch_loss() launches the engine's with the common arguments.  The
// tables below are the only places that name an instantiation: the launch and the LDS attribute of mvba_create both go through them.
template <typename... A>
struct LossKernel {
  void (*squared)(A...);
  void (*robust)(A..., LossArgs);
  const void *fn(bool rb) const { return rb ? (const void *)robust : (const void *)squared; }
};
template <typename... A>
LossKernel<A...> loss_kernel(void (*squared)(A...), void (*robust)(A..., LossArgs)) { return {squared, robust}; }

template <typename... A, typename... Args>
void launch_loss(mvba_handle *h, LossKernel<A...> k, dim3 grid, dim3 block, size_t lds, Args... args) {
  if (h->loss != LOSS_SQUARED) hipLaunchKernelGGL(k.robust, grid, block, lds, h->stream, args..., LossArgs{h->loss_b, h->d_sqw});
  else hipLaunchKernelGGL(k.squared, grid, block, lds, h->stream, args...);
}

// K1 and the cost pass: the robust instantiation is the one of the engine's loss (a squared engine never launches it)
auto resid_jac_kernel(bool gcam, int loss) {
  if (loss == LOSS_CAUCHY)
    return gcam ? loss_kernel(k_resid_jac<true>, k_resid_jac<true, LOSS_CAUCHY, LossArgs>) : loss_kernel(k_resid_jac<false>, k_resid_jac<false, LOSS_CAUCHY, LossArgs>);
  return gcam ? loss_kernel(k_resid_jac<true>, k_resid_jac<true, LOSS_HUBER, LossArgs>) : loss_kernel(k_resid_jac<false>, k_resid_jac<false, LOSS_HUBER, LossArgs>);
}
auto cost_kernel(bool gcam, int loss) {
  if (loss == LOSS_CAUCHY)
    return gcam ? loss_kernel(k_cost<true>, k_cost<true, LOSS_CAUCHY, LossArgs>) : loss_kernel(k_cost<false>, k_cost<false, LOSS_CAUCHY, LossArgs>);
  return gcam ? loss_kernel(k_cost<true>, k_cost<true, LOSS_HUBER, LossArgs>) : loss_kernel(k_cost<false>, k_cost<false, LOSS_HUBER, LossArgs>);
}
// K5: G lanes per point, bt threads per block (256 whenever the camera tables are in device memory)
template <int G>
auto backsub_kernel_g(int bt, bool gcam) {
  if (gcam) return loss_kernel(k_backsub<G, 256, true>, k_backsub<G, 256, true, true, LossArgs>);
  if (bt == 1024) return loss_kernel(k_backsub<G, 1024>, k_backsub<G, 1024, false, true, LossArgs>);
  if (bt == 512) return loss_kernel(k_backsub<G, 512>, k_backsub<G, 512, false, true, LossArgs>);
  return loss_kernel(k_backsub<G>, k_backsub<G, 256, false, true, LossArgs>);
}
auto backsub_kernel(int G, int bt, bool gcam) {
  return G == 2 ? backsub_kernel_g<2>(bt, gcam) : (G == 4 ? backsub_kernel_g<4>(bt, gcam) : backsub_kernel_g<8>(bt, gcam));
}
// K3, dense form: T tiles of 16 across the 9 m camera parameters; table: a point's records through d_dense_obs
template <int T>
auto dense_kernel_t(bool table) {
  return table ? loss_kernel(k_schur_dense<T, true>, k_schur_dense<T, true, true, LossArgs>)
               : loss_kernel(k_schur_dense<T, false>, k_schur_dense<T, false, true, LossArgs>);
}
auto dense_kernel(int T, bool table) {
  switch (T) {
    case 1: return dense_kernel_t<1>(table);
    case 2: return dense_kernel_t<2>(table);
    case 3: return dense_kernel_t<3>(table);
    case 4: return dense_kernel_t<4>(table);
    case 5: return dense_kernel_t<5>(table);
    case 6: return dense_kernel_t<6>(table);
    case 7: return dense_kernel_t<7>(table);
    case 8: return dense_kernel_t<8>(table);
    case 9: return dense_kernel_t<9>(table);
    case 10: return dense_kernel_t<10>(table);
    case 11: return dense_kernel_t<11>(table);
    default: return dense_kernel_t<12>(table);
  }
}
// its dynamic LDS for mm cameras (the launch: the engine's m; the attribute: the largest camera count of the instantiation)
size_t dense_lds_bytes(int T, int mm) {
  const int CH = dense_ch(T);
  return sizeof(double) * ((size_t)2 * 3 * CH * 16 * T + (size_t)2 * CH * mm * 32) + sizeof(double2) * CH * ((size_t)mm * REC + 8) +
         sizeof(double) * (CH * (size_t)mm + 2 * 3 * CH);
}

// dynamic LDS of K1 (the camera table, padded to 16 bytes, and 8 KiB of staging per wave) and of the kernels that hold the
// camera table alone (k_cost, k_residuals) or beside the camera steps (k_backsub); nothing once the tables are in device memory
size_t k1_lds_bytes(int m, bool gcam, int threads) {
  return (size_t)((gcam ? 0 : ((m * CAM_LDS + 1) & ~1)) + (threads / 64) * 64 * 2 * REC) * sizeof(double);
}
size_t cam_lds_bytes(int m, bool gcam, bool with_dxi) { return gcam ? 0 : (size_t)m * (CAM_LDS + (with_dxi ? DXI_LDS : 0)) * sizeof(double); }

// the camera tables in device memory for the kernels that cannot hold them in LDS (no-op up to LDS_CAMERAS cameras)
void cam_tables(mvba_handle *h, const double *cam15, const double *dxi) {
  if (h->gcam) hipLaunchKernelGGL(k_cam_tables, dim3((h->m + 255) / 256), dim3(256), 0, h->stream, h->m, cam15, dxi, h->f0, h->d_cam18, h->d_dxi10);
}
// the cost pass at a given state and the sum of its partials (into d_cost, and the mailbox when there is one)
int launch_cost(mvba_handle *h, const double *cam15, const double *X) {
  const size_t lds = cam_lds_bytes(h->m, h->gcam, false);
  cam_tables(h, cam15, nullptr);
  // (512 threads once the camera table leaves room for two blocks per CU only: config 4's 500 cameras)
  launch_loss(h, cost_kernel(h->gcam, h->loss), dim3(h->cost_grid), dim3(std::min(512, table_block_threads(lds))), lds, h->nobs, h->m, cam15, X,
              h->d_obs_pt, h->d_cam, h->d_xy, h->f0, h->d_partials, h->d_cam18);
  double *mail = cost_mail(h);  // (advances cost_seq: sequenced before the launch reads it)
  const unsigned long long seq = h->cost_seq;
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, h->stream, h->d_partials, h->cost_grid, h->d_cost, h->d_flag, mail, seq);
  MVBA_HIP(hipGetLastError());
  return MVBA_OK;
}

// The environment knobs of mvba_create (README.md lists them), read once.  Each pins a choice the engine otherwise makes
// by itself, or turns on a diagnostic that changes no result.
struct CreateKnobs {
  bool schur_set = false;                      // MVBA_SCHUR set at all (any value keeps a fully visible scene off the dense form
  bool schur_slots = false, schur_lanes = false, schur_pairs = false, schur_dense = false;  // ... unless it is `dense`)
  bool index_host = false, index_global = false;  // MVBA_INDEX=host | global: where the Schur index is built
  int slot_ranges = 0;                         // MVBA_SLOT_RANGES: the lane form's point ranges (0: counted from the wave places)
  bool force_big = false;                      // MVBA_FORCE_BIG
  bool rec_full = false;                       // MVBA_REC=full: the 128-byte record on a lane-form engine too
  bool chol_launches = false;                  // MVBA_CHOL=launches
  int trail64_min = 200;                       // MVBA_TRAIL64_MIN
  unsigned barrier_polls = 1u << 22;           // MVBA_CHOL_BARRIER_POLLS
  bool check_solve = false;                    // MVBA_CHECK_SOLVE=1 (or a tolerance in (0, 1))
  double check_solve_tol = 1e-8;
  bool timing = false;                         // MVBA_CREATE_TIMING=1: wall time of mvba_create's stages on stderr
};

CreateKnobs read_create_knobs() {
  CreateKnobs k;
  auto is = [](const char *ev, const char *v) { return ev && !strcmp(ev, v); };
  const char *schur = getenv("MVBA_SCHUR");
  k.schur_set = schur != nullptr;
  k.schur_slots = is(schur, "slots");
  k.schur_lanes = is(schur, "lanes");
  k.schur_pairs = is(schur, "pairs");
  k.schur_dense = is(schur, "dense");
  const char *index = getenv("MVBA_INDEX");
  k.index_host = is(index, "host");
  k.index_global = is(index, "global");
  if (const char *ev = getenv("MVBA_SLOT_RANGES")) k.slot_ranges = std::max(0, atoi(ev));
  k.force_big = getenv("MVBA_FORCE_BIG") != nullptr;
  k.rec_full = is(getenv("MVBA_REC"), "full");
  k.chol_launches = is(getenv("MVBA_CHOL"), "launches");
  if (const char *ev = getenv("MVBA_TRAIL64_MIN")) k.trail64_min = std::max(0, atoi(ev));
  if (const char *ev = getenv("MVBA_CHOL_BARRIER_POLLS")) k.barrier_polls = (unsigned)std::max(0LL, atoll(ev));
  if (const char *ev = getenv("MVBA_CHECK_SOLVE")) {
    const double v = atof(ev);
    k.check_solve = v != 0.0;
    if (v > 0.0 && v < 1.0) k.check_solve_tol = v;
  }
  k.timing = getenv("MVBA_CREATE_TIMING") != nullptr;
  return k;
}

}  // namespace
