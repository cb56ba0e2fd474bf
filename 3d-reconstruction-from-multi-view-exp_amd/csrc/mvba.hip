// libmvba.so -- bundle-adjustment engine for MI355X (gfx950), hand-written HIP.
//
// Replaces the numerical body of the reference's BundleAdjuster.optimize
// (lib/bundle_adjustment.py:103-162) with a sparse, observation-list pipeline:
//   K1  k_resid_jac      residual + 2x3 / 2x9 Jacobian rows per observation   (ref :291-427)
//   K2  (fused into K1)  E_a = 2 sum JxT Jx, dP_a = 2 sum JxT e               (ref :429-469, :519-556)
//   K3a k_point_inv      damped 3x3 inverse, v_a = E^-1 dP_a                  (ref :120-128)
//   K3  k_schur_slots | k_schur_lanes (up to ~100 cameras) / k_schur_pairs + k_schur_reduce / k_schur_dense (full visibility)
//                        A = G^ - sum F^T E^-1 F,  b = sum F^T E^-1 dP - dF   (ref :132-143, :471-517, :618-664)
//   C1  ncclAllReduce    [A|b] across point shards                            
//   K4  k_compact, k_chol_super / k_chol_trail64 / k_chol_trail32 / k_chol_backsolve_all (+ the k_lu_* rescue)
//                        dense solve of the gauge-reduced system              (ref :146)
//   K5+K6 k_backsub, k_cost  dX_a, trial state, trial cost                    (ref :152-162, :260-281, :666-677)
// HBM layout: observations sorted by point (CSR).  The linearisation of ONE
// observation is ONE 128-byte line ("record", 8 x double2 = (row0,row1) pairs):
//   slot 0-2  J_X columns          slot 3    dJ/df
//   slot 4-6  dJ/domega columns    slot 7    residual e
// J_C's translation columns are exactly -J_X and its (u,v) columns are the
// constants (1/f0,0),(0,1/f0) (ref :350-376), so the 2x9 block is implied by the
// record.  A point's observations are consecutive lines; the Schur kernel gathers whole lines
// (k-side record, l-side record, point block) per (point, camera pair) item.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "mvba_common.h"
#include "mvba_host.h"
#include "mvba_ransac_host.h"
#include "mvba_tracks_host.h"
#include "mvba_match_host.h"

namespace mvba {
thread_local std::string g_err;
}
using namespace mvba;

// ------------------------------------------------------------------ RCCL binding
// libmvba.so is NOT linked against librccl: a process may already hold one (PyTorch maps its own
// bundled librccl.so the moment torch.distributed creates a group), and two copies -- or headers of
// one release bound to the code of another by accident of load order -- is the version skew a
// collective library does not forgive.  The policy is explicit instead: use the librccl the
// process has ALREADY loaded if there is one (RTLD_NOLOAD), else load ROCm's; bind the seven entry
// points by name (all part of the NCCL 2.x C API: plain pointers, enums whose values have not
// changed since 2.0, the 128-byte id), and refuse a library whose major version differs from the
// headers this file was compiled against.  mvba_get_info reports both versions.
namespace {
struct Rccl {
  void *lib = nullptr;
  int version = 0;
  std::string origin;
  ncclResult_t (*GetVersion)(int *) = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;

int rccl_load() {
  if (g_rccl.lib) return MVBA_OK;
  const char *names[] = {"librccl.so.1", "librccl.so"};
  void *lib = nullptr;
  std::string origin;
  for (const char *n : names)
    if (!lib && (lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) origin = std::string(n) + " (already mapped by the process)";
  if (const char *ev = getenv("MVBA_RCCL_LIBRARY"))
    if (!lib && (lib = dlopen(ev, RTLD_NOW | RTLD_GLOBAL))) origin = ev;
  for (const char *n : {"/opt/rocm/lib/librccl.so.1", "librccl.so.1"})
    if (!lib && (lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) origin = n;
  if (!lib) return fail(MVBA_ERR_RCCL, std::string("librccl not found: ") + dlerror());
  Rccl r;
  r.lib = lib;
  r.origin = origin;
#define BIND(field, sym)                                                                       \
  if (!(r.field = reinterpret_cast<decltype(r.field)>(dlsym(lib, sym))))                       \
    return fail(MVBA_ERR_RCCL, std::string("librccl (") + origin + ") lacks " + sym)
  BIND(GetVersion, "ncclGetVersion");
  BIND(GetUniqueId, "ncclGetUniqueId");
  BIND(CommInitRank, "ncclCommInitRank");
  BIND(CommDestroy, "ncclCommDestroy");
  BIND(AllReduce, "ncclAllReduce");
  BIND(AllGather, "ncclAllGather");
  BIND(GetErrorString, "ncclGetErrorString");
#undef BIND
  if (r.GetVersion(&r.version) != ncclSuccess) return fail(MVBA_ERR_RCCL, "ncclGetVersion failed");
  // version code: major * 10000 + minor * 100 + patch since 2.9 (major * 1000 + ... before)
  const int major = r.version >= 10000 ? r.version / 10000 : r.version / 1000;
  if (major != NCCL_MAJOR)
    return fail(MVBA_ERR_RCCL, "librccl (" + origin + ") is NCCL " + std::to_string(r.version) + ", this library was built against " +
                                   std::to_string(NCCL_VERSION_CODE));
  g_rccl = r;
  return MVBA_OK;
}
}  // namespace

// ------------------------------------------------------------------ device code, one header per stage
namespace {

#include "mvba_device.h"     // what the stages share: fixed-order sums, the camera table in LDS, packed strips, REC / PBS
#include "mvba_linearize.h"  // K1 (+ K2), K3a: k_resid_jac, k_sum_split, k_point_inv
#include "mvba_schur.h"      // K3, the gather forms: k_schur_pairs*, k_schur_slots, k_schur_lanes (mvba_lanes.h), k_schur_reduce
#include "mvba_dense.h"      // K3, full visibility: k_schur_dense, k_schur_dense_finish
#include "mvba_solve.h"  // K4, device side: gauge strip, blocked Cholesky, the two back-substitutions, the pivoted-LU rescue
#include "mvba_tail.h"       // K5, K6 and the state kernels: k_backsub, k_cost, k_update_cams, k_cam_tables, k_residuals, ...
#include "mvba_index.h"      // the Schur index on the device: k_idx_*
#include "mvba_cov.h"  // marginal covariances (mvba_covariance): S^-1 from the Cholesky factor and the point pass
#include "mvba_map.h"  // parameter maps (mvba_set_parameter_map): the mapped gather into K4 and the way back

}  // namespace

// ------------------------------------------------------------------ host side
enum { SCHUR_PAIRS = 1, SCHUR_SLOTS = 2, SCHUR_DENSE = 3 };  // (0 was round 1's camera-strip form: the values are mvba_get_info's)
struct mvba_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  DevBufs mem;  // every device buffer below (h->mem.alloc): freed by mvba_destroy, or early by h->mem.release
  long long N = 0, nobs = 0;
  int m = 0, gauge_axis = 0, D = 0, ld = 0;
  double f0 = 1.0;
  // topology
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
  // pair-major Schur index (k_schur_pairs): items sorted by (k, l, point), units, per-XCD work queues
  bool use_pairs = true;              // pair-major index present (schur_mode != SCHUR_DENSE)
  int schur_mode = 2;                 // SCHUR_PAIRS / SCHUR_SLOTS (see k_schur_slots) / SCHUR_DENSE
  long long n_items = 0, n_items_offdiag = 0, n_slot_items = 0;
  int n_units = 0, rccl_version = 0, q_max = 0, n_waves = 0, slot_nR = 8, slot_nseg = 0;
  int slot_w = PSTEP;                 // slot form: lists per wave = items per step (21: k_schur_slots, 64: k_schur_lanes, not paced)
  long long *d_range_o0 = nullptr;    // slot form: first observation of every point range (the record base of its waves)
  int *d_seg_end = nullptr, *d_prog = nullptr;
  bool check_solve = false;           // MVBA_CHECK_SOLVE=1: every accepted dense solve is checked on the host against the packed system it solved
  double check_solve_tol = 1e-8;      // (MVBA_CHECK_SOLVE=<t> with 0 < t < 1: that tolerance -- the tests ask for an impossible one to see the check fire)
  bool gcam = false;                  // more than LDS_CAMERAS cameras: the kernels read the camera tables from device memory (d_cam18, d_dxi10)
  double *d_cam18 = nullptr, *d_dxi10 = nullptr;
  bool index_on_device = false;       // the Schur index was built by the k_idx_* kernels (nothing to upload)
  int4 *d_wdesc = nullptr;
  int *d_it_x = nullptr;              // slot form: the step-major index, 64 ints per step (k[21] | l[21] | a[21] | pad)
  int *d_wunits = nullptr;
  bool force_big = false;             // MVBA_FORCE_BIG: the 64-bit-offset kernels at any size
  int *d_it_k = nullptr, *d_it_l = nullptr, *d_it_a = nullptr, *d_unit_ptr = nullptr, *d_q_ptr = nullptr, *d_q_units = nullptr;
  int4 *d_units = nullptr;
  double *d_partial = nullptr;
  double *d_dense_part = nullptr;     // SCHUR_DENSE: partial tiles per workgroup
  int *d_dense_obs = nullptr;         // ... and, with missing observations, the observation of every (point, camera) or -1
  int dense_blocks = 0, dense_tiles = 0;
  // state: [cur] committed, [1-cur] trial
  double *d_X[2] = {nullptr, nullptr}, *d_cam15[2] = {nullptr, nullptr};
  int cur = 0;
  bool have_params = false, linearized = false, have_trial = false;
  // linearisation
  double2 *d_rec = nullptr;  // [n_obs][8] double2: one 128-B line per observation
  // the compact record (decided by mvba_create: lane form, squared loss, camera table in LDS, not MVBA_REC=full):
  // d_rec is [n_obs + 1][REC_C] -- J_X and d/df --, the residuals are d_res [n_obs + 1], PB carries X_a; d_rec_full is the full-layout
  // buffer mvba_covariance re-linearises into for its point pass, allocated on its first call
  bool rec_compact = false;
  double2 *d_res = nullptr, *d_rec_full = nullptr;
  double *d_PL = nullptr, *d_PB = nullptr;
  // reduced system: [A (9m x 9m) | b (9m)] contiguous for the all-reduce
  double *d_Ab = nullptr, *d_Ared = nullptr, *d_Ztiles = nullptr, *d_Lblk = nullptr, *d_dxi = nullptr, *d_dX = nullptr, *d_lu = nullptr;
  int *d_ipiv = nullptr;
  // cost
  double *d_partials = nullptr, *d_cost = nullptr, *h_cost = nullptr;
  double *d_mail = nullptr;               // device address of h_cost (pinned, mapped): the cost kernel's mailbox
  unsigned long long cost_seq = 0;
  bool mail_pending = false;
  int n_partials = 0, cost_grid = 0;
  int *d_flag = nullptr, *h_flag = nullptr;
  unsigned *d_bar = nullptr;
  int n_cu = 1;
  bool chol_onepass = true;  // L^T x = y as one persistent launch (MVBA_CHOL=launches: one launch per super-block)
  int trail64_min = 200;     // trailing updates of at least this many 64 x 64 workgroups run k_chol_trail64 (MVBA_TRAIL64_MIN)
  unsigned barrier_polls = 1u << 22;  // what a wait of that launch polls before it gives up (MVBA_CHOL_BARRIER_POLLS)
  // comm
  ncclComm_t comm = nullptr;
  mvba_host_allreduce_fn host_ar = nullptr;  // host-staged transport (mvba_comm_init_host) instead of RCCL
  void *host_ar_user = nullptr;
  std::vector<double> host_buf;
  int rank = 0, nranks = 1;
  double *d_allcost = nullptr, *h_allcost = nullptr, *d_sim = nullptr;
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
  double2 *d_resid = nullptr;  // mvba_residuals, allocated on the first call
  double *d_init_cams = nullptr;  // mvba_triangulate_state, allocated on the first call: the committed cameras as K, R, t ([m][9 + 9 + 3])
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
  launch_loss(h, cost_kernel(h->gcam, h->loss), dim3(h->cost_grid), dim3(lds > 40 * 1024 ? 512 : 256), lds, h->nobs, h->m, cam15, X,
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

#include "mvba_create.h"  // engine creation as stages: create_engine()

}  // namespace

extern "C" {

const char *mvba_version(void) { return "mvba 0.2 (gfx950)"; }
const char *mvba_last_error(void) { return g_err.c_str(); }
const char *mvba_kernel_name(int32_t k) { return (k >= 0 && k < MVBA_K_COUNT) ? kKernelNames[k] : ""; }

int mvba_device_count(int32_t *count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(MVBA_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = n;
  return MVBA_OK;
}

int mvba_create(const mvba_problem *p, mvba_handle **out) { return create_engine(p, LOSS_SQUARED, 0.0, out); }

int mvba_create_robust(const mvba_problem *p, int32_t loss, double scale, mvba_handle **out) {
  if (!p || !out) return fail(MVBA_ERR_BADARG, "null argument");
  if (loss == LOSS_SQUARED) return create_engine(p, LOSS_SQUARED, 0.0, out);
  if (loss != LOSS_HUBER && loss != LOSS_CAUCHY)
    return fail(MVBA_ERR_BADARG, "loss = " + std::to_string(loss) + " is not a loss (0 squared, 1 Huber, 2 Cauchy)");
  if (!(scale > 0.0) || !std::isfinite(scale))
    return fail(MVBA_ERR_BADARG, "loss scale = " + std::to_string(scale) + " must be finite and > 0 for a robust loss");
  if (!(p->f0 > 0.0) || !std::isfinite(p->f0)) return fail(MVBA_ERR_BADARG, "a robust loss needs f0 > 0");
  const double r = scale / p->f0;
  return create_engine(p, loss, r * r, out);
}

void mvba_destroy(mvba_handle *h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->comm) g_rccl.CommDestroy(h->comm);
  h->mem.release_all();
  if (h->h_cost) hipHostFree(h->h_cost);
  if (h->h_allcost) hipHostFree(h->h_allcost);
  for (auto &p : h->pending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
  for (auto e : h->pool) hipEventDestroy(e);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
}

// ---- cam15, the engine's camera row: f | u (2) | t (3) | R (9, row-major) -- to and from the C interface's arrays
namespace {
void pack_cam15(int m, const double *f, const double *u, const double *t, const double *R, double *cam /*[m][CAM_IN]*/) {
  for (int k = 0; k < m; ++k) {
    double *c = cam + (size_t)k * CAM_IN;
    c[0] = f[k]; c[1] = u[2 * k]; c[2] = u[2 * k + 1];
    for (int i = 0; i < 3; ++i) c[3 + i] = t[3 * k + i];
    for (int i = 0; i < 9; ++i) c[6 + i] = R[9 * k + i];
  }
}
void unpack_cam15(const double *cam /*[m][CAM_IN]*/, int m, double *f, double *u, double *t, double *R) {
  for (int k = 0; k < m; ++k) {
    const double *c = cam + (size_t)k * CAM_IN;
    f[k] = c[0]; u[2 * k] = c[1]; u[2 * k + 1] = c[2];
    for (int i = 0; i < 3; ++i) t[3 * k + i] = c[3 + i];
    for (int i = 0; i < 9; ++i) R[9 * k + i] = c[6 + i];
  }
}
}  // namespace

int mvba_set_params(mvba_handle *h, const double *X, const double *f, const double *u, const double *t, const double *R) {
  if (!h || !X || !f || !u || !t || !R) return fail(MVBA_ERR_BADARG, "null argument");
  MVBA_HIP(hipSetDevice(h->device));
  std::vector<double> cam((size_t)h->m * CAM_IN);
  pack_cam15(h->m, f, u, t, R, cam.data());
  MVBA_HIP(hipMemcpyAsync(h->d_X[h->cur], X, sizeof(double) * 3 * h->N, hipMemcpyHostToDevice, h->stream));
  MVBA_HIP(hipMemcpyAsync(h->d_cam15[h->cur], cam.data(), sizeof(double) * cam.size(), hipMemcpyHostToDevice, h->stream));
  MVBA_HIP(hipStreamSynchronize(h->stream));
  h->have_params = true; h->linearized = false; h->have_trial = false;
  return MVBA_OK;
}

int mvba_get_params(mvba_handle *h, double *X, double *f, double *u, double *t, double *R) {
  if (!h || !X || !f || !u || !t || !R) return fail(MVBA_ERR_BADARG, "null argument");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set");
  MVBA_HIP(hipSetDevice(h->device));
  std::vector<double> cam((size_t)h->m * CAM_IN);
  MVBA_HIP(hipMemcpyAsync(X, h->d_X[h->cur], sizeof(double) * 3 * h->N, hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipMemcpyAsync(cam.data(), h->d_cam15[h->cur], sizeof(double) * cam.size(), hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipStreamSynchronize(h->stream));
  unpack_cam15(cam.data(), h->m, f, u, t, R);
  return MVBA_OK;
}

int mvba_apply_similarity(mvba_handle *h, const double *R0, const double *t0, double scale) {
  if (!h || !R0 || !t0) return fail(MVBA_ERR_BADARG, "null argument");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set");
  MVBA_HIP(hipSetDevice(h->device));
  double T[13];
  memcpy(T, R0, 9 * sizeof(double));
  memcpy(T + 9, t0, 3 * sizeof(double));
  T[12] = scale;
  if (!h->d_sim) {
    int rc = h->mem.alloc(&h->d_sim, 13);
    if (rc) return rc;
  }
  MVBA_HIP(hipMemcpyAsync(h->d_sim, T, sizeof(T), hipMemcpyHostToDevice, h->stream));
  const long long n = std::max<long long>(h->N, h->m);
  hipLaunchKernelGGL(k_similarity, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->N, h->m, h->d_X[h->cur],
                     h->d_cam15[h->cur], h->d_sim);
  MVBA_HIP(hipGetLastError());
  MVBA_HIP(hipStreamSynchronize(h->stream));  // T lives on this frame's stack
  h->linearized = false; h->have_trial = false;
  return MVBA_OK;
}

int mvba_cost(mvba_handle *h, double *E) {
  if (!h || !E) return fail(MVBA_ERR_BADARG, "null argument");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set");
  MVBA_HIP(hipSetDevice(h->device));
  {
    Timed t(h, MVBA_K_COST);
    int rc = launch_cost(h, h->d_cam15[h->cur], h->d_X[h->cur]);
    if (rc) return rc;
  }
  return global_cost(h, E);
}

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
  const int m = h->m;
  const size_t n9 = 9 * (size_t)m, nA = strip_offset(m, m);
  const long long nAb = (long long)(nA + n9);
  const unsigned grid = (unsigned)std::max<long long>((h->N + 255) / 256, std::min<long long>((nAb + 1023) / 1024, 4096));
  const long long nprog = h->slot_w == LANES_W ? 0 : (long long)h->slot_nR * h->slot_nseg * PACE_STRIDE;
  const int want_r = h->schur_mode == SCHUR_DENSE ? 1 : 0;
  const double *Xc = h->rec_compact ? h->d_X[h->cur] : nullptr;  // a compact engine's point rows carry X_a (the state K1 linearised at)
  if (h->n_held)  // held points (mvba_set_point_hold): the masked form; without a mask the launch is the one it always was
    hipLaunchKernelGGL(k_point_inv<const uint8_t *>, dim3(std::max(grid, 1u)), dim3(256), 0, h->stream, h->N, c, h->d_PL, h->d_PB, h->d_flag,
                       h->d_Ab, nAb, h->d_prog, nprog, want_r, Xc, (const uint8_t *)h->d_held);
  else
    hipLaunchKernelGGL(k_point_inv<>, dim3(std::max(grid, 1u)), dim3(256), 0, h->stream, h->N, c, h->d_PL, h->d_PB, h->d_flag,
                       h->d_Ab, nAb, h->d_prog, nprog, want_r, Xc);
}

void launch_schur(mvba_handle *h, double c) {  // K3 in the engine's form: [A|b] of this rank's points
  const int m = h->m;
  const size_t nA = strip_offset(m, m);
  double *d_A = h->d_Ab, *d_b = h->d_Ab + nA;
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
    const long long n_el = (long long)nA + 9 * m;
    hipLaunchKernelGGL(k_schur_dense_finish, dim3((unsigned)((n_el + 3) / 4)), dim3(256), 0, h->stream, m, T, h->dense_blocks,
                       (const double *)h->d_dense_part, c, d_A, d_b);
  }
}

int allreduce_Ab(mvba_handle *h, bool timed) {  // C1: [A|b] summed over the ranks (RCCL or the host transport)
  const int m = h->m;
  const size_t n9 = 9 * (size_t)m, nA = strip_offset(m, m);
  if (h->comm) {
    Timed t(h, timed ? MVBA_K_ALLREDUCE : -1);
    ncclResult_t r = g_rccl.AllReduce(h->d_Ab, h->d_Ab, nA + n9, ncclDouble, ncclSum, h->comm, h->stream);
    if (r != ncclSuccess) return fail(MVBA_ERR_RCCL, std::string("ncclAllReduce: ") + g_rccl.GetErrorString(r));
  } else if (h->host_ar) {  // host-staged transport: D2H, caller's sum, H2D (no RCCL; see mvba_comm_init_host)
    h->host_buf.resize(nA + n9);
    MVBA_HIP(hipMemcpyAsync(h->host_buf.data(), h->d_Ab, sizeof(double) * (nA + n9), hipMemcpyDeviceToHost, h->stream));
    MVBA_HIP(hipStreamSynchronize(h->stream));
    const auto t0 = std::chrono::steady_clock::now();  // the wait above belongs to the Schur kernel, not to the exchange
    if (h->host_ar(h->host_ar_user, h->host_buf.data(), (int64_t)(nA + n9))) return fail(MVBA_ERR_RCCL, "host all-reduce callback failed");
    MVBA_HIP(hipMemcpyAsync(h->d_Ab, h->host_buf.data(), sizeof(double) * (nA + n9), hipMemcpyHostToDevice, h->stream));
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
  double *d_A = h->d_Ab, *d_b = h->d_Ab + strip_offset(m, m);
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

namespace {
// The pieces of the LM trial (mvba_try_step below reads as the step).
// With a parameter map the solve kernels run on the D' x D' mapped system and scatter x (through keep_index, as ever) into a
// scratch vector; k_map_expand then writes dxi = P x.  D' = 0 (everything held): dxi = 0, no solve.
double *solve_x(mvba_handle *h) { return h->mapped ? h->d_map_x : h->d_dxi; }
void launch_expand(mvba_handle *h) {
  const size_t n9 = 9 * (size_t)h->m;
  if (h->mapped && h->solve_D() > 0)
    hipLaunchKernelGGL(k_map_expand, dim3((unsigned)((n9 + 255) / 256)), dim3(256), 0, h->stream, (int)n9, h->gauge_axis, h->d_map_col,
                       h->d_map_x, h->d_dxi);
}

void launch_solve(mvba_handle *h, bool onepass) {  // K4: gauge strip, blocked Cholesky, back-substitution
  const int m = h->m, D = h->solve_D();
  double *d_x = solve_x(h);
  Timed t(h, MVBA_K_SOLVE);
  if (D == 0) {  // (only with a map)
    hipMemsetAsync(h->d_dxi, 0, sizeof(double) * 9 * (size_t)m, h->stream);
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
  double *d_A = h->d_Ab, *d_b = h->d_Ab + strip_offset(m, m), *d_x = solve_x(h);
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
      const double deg = (double)h->nobs / (double)h->N;  // lanes per point by mean degree
      const int G = deg <= 40.0 ? 2 : (deg <= 100.0 ? 4 : 8);
      // (a camera table above half the LDS leaves one block per CU: 1024 threads then, so that the CU still holds 16 waves)
      // (16 waves per CU is what the registers allow: 256-thread blocks reach it while four of them fit -- tables up to 40 KiB,
      // ~180 cameras --, 512-thread blocks while two fit, one 1024-thread block beyond)
      const int bt = lds > 80 * 1024 ? 1024 : (lds > 40 * 1024 ? 512 : 256);
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
// plain loops.  The persistent back-substitution orders its hand-overs with sc1 accesses and explicit waits, not with the
// memory model's fences: a stale read there would be a silently wrong camera step, which this catches.
int check_solve_residual(mvba_handle *h) {
  const int m = h->m, D = h->solve_D();
  const size_t n9 = 9 * (size_t)m, nA = strip_offset(m, m);
  std::vector<double> Ab(nA + n9), x(n9);
  MVBA_HIP(hipMemcpyAsync(Ab.data(), h->d_Ab, sizeof(double) * (nA + n9), hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipMemcpyAsync(x.data(), h->d_dxi, sizeof(double) * n9, hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipStreamSynchronize(h->stream));
  auto kept = [&](size_t g) { return !((g >= 3 && g <= 8) || g == (size_t)(12 + h->gauge_axis)); };
  std::vector<double> r(n9, 0.0), an(n9, 0.0);  // r = A x, an = |A| |x|  (rows of the full symmetric matrix from the packed upper strips)
  for (int k = 0; k < m; ++k) {
    const double *Ak = Ab.data() + strip_offset(k, m);
    const int Wk = 9 * (m - k);
    for (int i = 0; i < 9; ++i)
      for (int c = 0; c < Wk; ++c) {
        const size_t gi = 9 * (size_t)k + i, gj = 9 * (size_t)k + c;
        const double a = Ak[(size_t)i * Wk + c];
        r[gi] += a * x[gj]; an[gi] += std::fabs(a * x[gj]);
        if (c >= 9) { r[gj] += a * x[gi]; an[gj] += std::fabs(a * x[gi]); }  // the mirror image below the diagonal blocks
      }
  }
  double worst = 0.0;
  if (h->mapped) {  // the mapped system's residual P^T (b - A P x): x above is dxi = P x, rows summed over an unknown's members
    for (int j = 0; j < D; ++j) {
      double res = 0.0, scale = 0.0;
      for (int q = h->map_ptr[j]; q < h->map_ptr[j + 1]; ++q) {
        const size_t g = (size_t)h->map_mem[q];
        res += Ab[nA + g] - r[g];
        scale += an[g] + std::fabs(Ab[nA + g]);
      }
      worst = std::max(worst, scale > 0.0 ? std::fabs(res) / scale : 0.0);
    }
  } else
  for (size_t g = 0; g < n9; ++g)
    if (kept(g)) {
      const double bg = Ab[nA + g], scale = an[g] + std::fabs(bg);
      worst = std::max(worst, scale > 0.0 ? std::fabs(bg - r[g]) / scale : 0.0);
    }
  if (!(worst <= h->check_solve_tol))
    return fail(MVBA_ERR_STATE, "MVBA_CHECK_SOLVE: the dense solve left a relative residual of " + std::to_string(worst) +
                                    " on the reduced camera system (a stale hand-over in the back-substitution?)");
  return MVBA_OK;
}
}  // namespace

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

int mvba_set_parameter_map(mvba_handle *h, const int32_t *col, int32_t n_free) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  MVBA_HIP(hipSetDevice(h->device));
  const int m = h->m, n9 = 9 * m;
  auto is_gauge = [&](int g) { return (g >= 3 && g <= 8) || g == 12 + h->gauge_axis; };
  if (!col) {  // the default map: the seven gauge slots held, everything else free
    h->mapped = false;
    h->have_trial = false;
    return MVBA_OK;
  }
  if (n_free < 0 || n_free > h->D)
    return fail(MVBA_ERR_BADARG, "mvba_set_parameter_map: n_free = " + std::to_string(n_free) + " must be in 0 .. 9 n_images - 7 = " + std::to_string(h->D));
  std::vector<int> cnt(n_free + 1, 0), first(n_free, -1);
  for (int g = 0; g < n9; ++g) {
    const int j = col[g];
    if (j < -1 || j >= n_free)
      return fail(MVBA_ERR_BADARG, "mvba_set_parameter_map: col[" + std::to_string(g) + "] = " + std::to_string(j) + " is neither -1 nor below n_free = " + std::to_string(n_free));
    if (j >= 0 && is_gauge(g))
      return fail(MVBA_ERR_BADARG, "mvba_set_parameter_map: col[" + std::to_string(g) + "] is a gauge slot and must be -1");
    if (j < 0) continue;
    if (first[j] < 0) first[j] = g;
    else if (g % 9 != first[j] % 9 || g % 9 > 2)
      return fail(MVBA_ERR_BADARG, "mvba_set_parameter_map: col[" + std::to_string(g) + "] ties slot " + std::to_string(g) + " to slot " + std::to_string(first[j]) +
                                       " (unknown " + std::to_string(j) + "): only the same intrinsic parameter (f, u or v) of different cameras can be tied");
    ++cnt[j];
  }
  for (int j = 0; j < n_free; ++j)
    if (!cnt[j]) return fail(MVBA_ERR_BADARG, "mvba_set_parameter_map: unknown " + std::to_string(j) + " has no parameter slot");
  bool is_default = n_free == h->D;
  for (int g = 0, j = 0; is_default && g < n9; ++g) is_default = col[g] == (is_gauge(g) ? -1 : j++);
  h->have_trial = false;
  if (is_default) {  // spelled out: the engine runs exactly what it runs without a map
    h->mapped = false;
    return MVBA_OK;
  }
  std::vector<int> ptr(n_free + 1, 0), mem;
  for (int j = 0; j < n_free; ++j) ptr[j + 1] = ptr[j] + cnt[j];
  mem.resize(std::max(ptr[n_free], 1));
  {
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int g = 0; g < n9; ++g)
      if (col[g] >= 0) mem[fill[col[g]]++] = g;  // ascending g within an unknown
  }
  int U = 0;
  while (U < n_free && cnt[U] == 1) ++U;
  // the tied x tied entries of the lower triangle, and how many workgroups share one: eight of the row's members each, 64 at most
  std::vector<int2> pairs;
  int max_cnt = 1;
  {
    std::vector<int> tied;
    for (int j = 0; j < n_free; ++j)
      if (cnt[j] > 1) { tied.push_back(j); max_cnt = std::max(max_cnt, cnt[j]); }
    for (size_t a = 0; a < tied.size(); ++a)
      for (size_t b = 0; b <= a; ++b) pairs.push_back(make_int2(tied[a], tied[b]));
  }
  const int nblk = std::min(64, (max_cnt + 7) / 8);
  int2 *d_pairs = nullptr;
  double *d_part = nullptr;
  if (!pairs.empty()) {
    int rc = h->mem.alloc(&d_pairs, pairs.size());
    if (!rc) rc = h->mem.alloc(&d_part, pairs.size() * (size_t)nblk);
    if (rc) {
      h->mem.release(d_pairs);
      return rc;
    }
  }
  if (!h->d_map_col) {
    int rc = h->mem.alloc(&h->d_map_col, (size_t)n9);
    if (!rc) rc = h->mem.alloc(&h->d_map_ptr, (size_t)h->D + 1);
    if (!rc) rc = h->mem.alloc(&h->d_map_mem, (size_t)n9);
    if (!rc) rc = h->mem.alloc(&h->d_map_x, (size_t)n9 + 16);  // (the back-substitution clears 9m slots, or slots 3..8 and 12 + axis)
    if (rc) {
      h->mem.release(h->d_map_col); h->mem.release(h->d_map_ptr); h->mem.release(h->d_map_mem); h->mem.release(h->d_map_x);
      h->mem.release(d_pairs); h->mem.release(d_part);
      return rc;
    }
  }
  MVBA_HIP(hipStreamSynchronize(h->stream));  // nothing in flight reads the tables that are replaced now
  h->mem.release(h->d_map_pairs);
  h->mem.release(h->d_map_part);
  h->d_map_pairs = d_pairs;
  h->d_map_part = d_part;
  h->n_map_pairs = (int)pairs.size();
  h->map_nblk = nblk;
  if (!pairs.empty()) MVBA_HIP(hipMemcpy(h->d_map_pairs, pairs.data(), sizeof(int2) * pairs.size(), hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(h->d_map_col, col, sizeof(int) * n9, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(h->d_map_ptr, ptr.data(), sizeof(int) * (n_free + 1), hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(h->d_map_mem, mem.data(), sizeof(int) * mem.size(), hipMemcpyHostToDevice));
  h->map_col.assign(col, col + n9);
  h->map_ptr = ptr;
  h->map_mem = mem;
  h->n_free = n_free;
  h->map_ld = (n_free + 3) & ~3;
  h->map_U = U;
  h->mapped = true;
  return MVBA_OK;
}

int mvba_set_point_hold(mvba_handle *h, const uint8_t *held) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  MVBA_HIP(hipSetDevice(h->device));
  long long n_held = 0;
  std::vector<uint8_t> mask;
  if (held) {
    mask.resize((size_t)h->N);
    for (long long a = 0; a < h->N; ++a) n_held += (mask[(size_t)a] = held[a] ? 1 : 0);
  }
  if (n_held && !h->d_held) {
    int rc = h->mem.alloc(&h->d_held, (size_t)h->N);
    if (rc) return rc;
  }
  if (n_held) {
    MVBA_HIP(hipStreamSynchronize(h->stream));  // nothing in flight reads the mask that is replaced now
    MVBA_HIP(hipMemcpy(h->d_held, mask.data(), mask.size(), hipMemcpyHostToDevice));
  }
  h->n_held = n_held;  // (no held point, spelled out or NULL: the engine runs exactly what it runs without a mask)
  h->have_trial = false;
  return MVBA_OK;
}

int mvba_residuals(mvba_handle *h, double *e) {
  if (!h || !e) return fail(MVBA_ERR_BADARG, "null argument");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set");
  MVBA_HIP(hipSetDevice(h->device));
  if (!h->nobs) return MVBA_OK;
  if (!h->d_resid) {
    int rc = h->mem.alloc(&h->d_resid, h->nobs);
    if (rc) return rc;
  }
  const size_t lds = cam_lds_bytes(h->m, h->gcam, false);
  cam_tables(h, h->d_cam15[h->cur], nullptr);
  const unsigned grid = (unsigned)std::min<long long>(4096, (h->nobs + 255) / 256);
  hipLaunchKernelGGL(h->gcam ? k_residuals<true> : k_residuals<false>, dim3(grid), dim3(256), lds, h->stream, h->nobs, h->m,
                     (const double *)h->d_cam15[h->cur], (const double *)h->d_X[h->cur], (const int *)h->d_obs_pt, (const int *)h->d_cam,
                     (const double2 *)h->d_xy, h->f0, h->d_resid, (const double *)h->d_cam18);
  MVBA_HIP(hipGetLastError());
  MVBA_HIP(hipMemcpyAsync(e, h->d_resid, sizeof(double2) * h->nobs, hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipStreamSynchronize(h->stream));
  return MVBA_OK;
}

int mvba_covariance(mvba_handle *h, double *point_cov, double *cam_cov, double *cam_cov_full, double *timings_ms) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  if (h->loss != LOSS_SQUARED)
    return fail(MVBA_ERR_BADARG, "mvba_covariance: the covariance is defined for the squared loss only (this engine has a robust loss)");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set");
  MVBA_HIP(hipSetDevice(h->device));
  const int m = h->m, D = h->solve_D(), ld = h->solve_ld(), nt = (D + NB - 1) / NB;
  const size_t n_sig = sig_block(m, m, m);  // (the block index of (m, m) is the block count)
  // First call: the camera-block table, the trtri panels, the point and camera blocks -- all four or none (a failed
  // allocation frees what it got, so that a later call never runs with some of them missing)
  auto free_cov = [&]() {
    for (double **q : {&h->d_cov_sig, &h->d_cov_panel, &h->d_cov_pts, &h->d_cov_cam}) h->mem.release(*q);
  };
  int local_rc = MVBA_OK;
  if (!h->d_cov_sig || !h->d_cov_panel || !h->d_cov_pts || !h->d_cov_cam) {
    free_cov();
    local_rc = h->mem.alloc(&h->d_cov_sig, n_sig);
    if (!local_rc) local_rc = h->mem.alloc(&h->d_cov_panel, 2 * (size_t)h->D * NB);
    if (!local_rc) local_rc = h->mem.alloc(&h->d_cov_pts, 6 * (size_t)h->N);
    if (!local_rc) local_rc = h->mem.alloc(&h->d_cov_cam, 81 * (size_t)m);
    if (local_rc) free_cov();
  }
  hipEvent_t ev[5] = {};
  struct EvFree { hipEvent_t *e; ~EvFree() { for (int i = 0; i < 5; ++i) if (e[i]) hipEventDestroy(e[i]); } } ev_free{ev};
  for (auto &e : ev)
    if (!local_rc && hipEventCreate(&e) != hipSuccess) local_rc = fail(MVBA_ERR_HIP, "hipEventCreate failed");
  // With a parameter map k_cov_lauum scatters Sigma' (D' x D') through keep_index into a scratch table of mv camera blocks per side
  // (mv <= m); k_map_cov_expand then fills the real table with P Sigma' P^T.
  const int mv = (D + 6) / 9 + 1;
  if (!local_rc && h->mapped && D > 0 && !h->d_cov_sigv) local_rc = h->mem.alloc(&h->d_cov_sigv, n_sig);
  // A compact engine: the point pass reads J_omega of both observations of a pair -- it gets full-layout records of its own, from a
  // second K1 launch below (the same E_a and dP_a once more), rather than a second layout of k_point_cov
  if (!local_rc && h->rec_compact && point_cov && h->nobs && !h->d_rec_full) local_rc = h->mem.alloc(&h->d_rec_full, (size_t)REC * h->nobs);
  const bool sharded = h->comm || h->host_ar;
  if (local_rc && !sharded) return local_rc;
  const std::string local_err = local_rc ? g_err : std::string();
  double *d_b = h->d_Ab + strip_offset(m, m);
  if (!local_rc) {
    MVBA_HIP(hipEventRecord(ev[0], h->stream));
    // 1-4: the LM step's launches at c = 0 (K1, K3a, K3 in the engine's form, the all-reduce of [A|b])
    if (h->nobs && h->rec_compact && point_cov) launch_resid_jac(h, h->d_rec_full);
    if (h->nobs) launch_resid_jac(h);
    h->linearized = true; h->have_trial = false;
    launch_point_inv(h, 0.0);
    launch_schur(h, 0.0);
    MVBA_HIP(hipGetLastError());
  } else {
    // A rank that could not set up still takes part in the collective (the others would wait in it for ever): it marks
    // b[3] -- camera 0's t_x, a gauge slot the solve never reads -- with a NaN (all-ones bytes), so that every rank sees
    // it in the sum and fails the call with it.
    MVBA_HIP(hipMemsetAsync(d_b + 3, 0xFF, sizeof(double), h->stream));
  }
  {
    int rc = allreduce_Ab(h, false);
    if (rc) return rc;
  }
  if (sharded) {
    double mark = 0.0;
    MVBA_HIP(hipMemcpyAsync(&mark, d_b + 3, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MVBA_HIP(hipStreamSynchronize(h->stream));
    if (local_rc) return fail(local_rc, local_err);
    if (std::isnan(mark))
      return fail(MVBA_ERR_HIP, "mvba_covariance: another rank could not allocate its covariance buffers (or the reduced system is not finite)");
  }
  MVBA_HIP(hipEventRecord(ev[1], h->stream));
  // 5: gauge strip + blocked Cholesky of the undamped S
  if (D > 0) launch_factor(h);
  MVBA_HIP(hipEventRecord(ev[2], h->stream));
  // 6a: W = L^-1 in place in d_Ared, then Sigma = W^T W into the camera-block table (zeros at the gauge slots)
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
  MVBA_HIP(hipMemsetAsync(h->d_cov_sig, 0, sizeof(double) * n_sig, h->stream));
  if (h->mapped) {
    if (D > 0) {
      hipLaunchKernelGGL(k_cov_lauum, dim3(nt * (nt + 1) / 2), dim3(256), 0, h->stream, (const double *)h->d_Ared, ld, D, nt, mv,
                         h->gauge_axis, h->d_cov_sigv);
      hipLaunchKernelGGL(k_map_cov_expand, dim3((unsigned)((81 * m + 255) / 256), m), dim3(256), 0, h->stream, m, mv, h->gauge_axis,
                         (const int *)h->d_map_col, (const double *)h->d_cov_sigv, h->d_cov_sig);
    }
  } else
  hipLaunchKernelGGL(k_cov_lauum, dim3(nt * (nt + 1) / 2), dim3(256), 0, h->stream, (const double *)h->d_Ared, ld, D, nt, m,
                     h->gauge_axis, h->d_cov_sig);
  MVBA_HIP(hipEventRecord(ev[3], h->stream));
  // 6b: the point pass and the camera blocks
  if (h->N && point_cov) {
    const double pairs = h->N ? 0.5 * ((double)h->nobs / (double)h->N) * ((double)h->nobs / (double)h->N + 1.0) : 0.0;
    const int G = pairs > 48.0 ? 64 : (pairs > 24.0 ? 32 : (pairs > 12.0 ? 16 : 8));  // lanes per point by mean pair count
    const unsigned grid = (unsigned)std::min<long long>(8192, (h->N * G + 255) / 256);
    auto launch = [&](auto kern, auto... held) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, h->stream, h->N, m, (const long long *)h->d_pt_ptr, (const int *)h->d_cam,
                         (const double2 *)(h->rec_compact ? h->d_rec_full : h->d_rec), (const double *)h->d_PL, (const double *)h->d_cov_sig, 1.0 / h->f0, h->d_cov_pts,
                         h->d_flag, held...);
    };
    if (h->n_held) {  // held points skip the pair loop and the pivot test: six zeros
      using M = const uint8_t *;
      launch(G == 64 ? k_point_cov<64, M> : (G == 32 ? k_point_cov<32, M> : (G == 16 ? k_point_cov<16, M> : k_point_cov<8, M>)), (M)h->d_held);
    } else
      launch(G == 64 ? k_point_cov<64> : (G == 32 ? k_point_cov<32> : (G == 16 ? k_point_cov<16> : k_point_cov<8>)));
  }
  if (cam_cov)
    hipLaunchKernelGGL(k_cov_cam_diag, dim3((unsigned)((81LL * m + 255) / 256)), dim3(256), 0, h->stream, m,
                       (const double *)h->d_cov_sig, h->d_cov_cam);
  MVBA_HIP(hipGetLastError());
  MVBA_HIP(hipEventRecord(ev[4], h->stream));
  int fl = 0;
  MVBA_HIP(hipMemcpyAsync(&fl, h->d_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipStreamSynchronize(h->stream));
  if (fl) {
    MVBA_HIP(hipMemsetAsync(h->d_flag, 0, sizeof(int), h->stream));
    MVBA_HIP(hipStreamSynchronize(h->stream));
    if (fl & (FLAG_POINT_SINGULAR | FLAG_COV_POINT)) return fail(MVBA_ERR_SINGULAR, "Singular matrix (a point block E_a is singular: a point seen once, or without parallax)");
    return fail(MVBA_ERR_SINGULAR, "Singular matrix (the undamped reduced camera system is not positive definite)");
  }
  if (timings_ms)
    for (int i = 0; i < 4; ++i) {
      float ms = 0.f;
      MVBA_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
      timings_ms[i] = ms;
    }
  if (point_cov && h->N) MVBA_HIP(hipMemcpy(point_cov, h->d_cov_pts, sizeof(double) * 6 * h->N, hipMemcpyDeviceToHost));
  if (cam_cov) MVBA_HIP(hipMemcpy(cam_cov, h->d_cov_cam, sizeof(double) * 81 * m, hipMemcpyDeviceToHost));
  if (cam_cov_full) {  // the table, expanded on the host strip by strip (blocks (k, k..m-1) are contiguous): C = 2 S^-1, both triangles
    std::vector<double> strip((size_t)SIG_BS * m);
    const size_t n9 = 9 * (size_t)m;
    for (int k = 0; k < m; ++k) {
      MVBA_HIP(hipMemcpy(strip.data(), h->d_cov_sig + sig_block(k, k, m), sizeof(double) * SIG_BS * (m - k), hipMemcpyDeviceToHost));
      for (int l = k; l < m; ++l) {
        const double *b = strip.data() + (size_t)SIG_BS * (l - k);
        for (int i = 0; i < 9; ++i)
          for (int j = 0; j < 9; ++j) {
            const double v = 2.0 * b[9 * i + j];
            cam_cov_full[(9 * (size_t)k + i) * n9 + 9 * (size_t)l + j] = v;
            cam_cov_full[(9 * (size_t)l + j) * n9 + 9 * (size_t)k + i] = v;
          }
      }
    }
  }
  return MVBA_OK;
}

// ---- debug log: per-iteration copies of the committed state, device-resident (ref :89-98, :175-183, :204-206)
namespace {
constexpr int SNAP_SLAB = 8;  // log entries per device allocation
size_t snap_stride(const mvba_handle *h) { return (3 * (size_t)h->N + (size_t)CAM_IN * h->m + 1) & ~(size_t)1; }
// log entry i: points [3 N], then cameras [m][CAM_IN] (its slab must exist)
double *snap_entry(const mvba_handle *h, long long i) { return h->snap_slabs[(size_t)(i / SNAP_SLAB)] + snap_stride(h) * (size_t)(i % SNAP_SLAB); }
}  // namespace

int mvba_snapshot(mvba_handle *h) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set");
  MVBA_HIP(hipSetDevice(h->device));
  if ((size_t)(h->n_snap / SNAP_SLAB) >= h->snap_slabs.size()) {
    double *p = nullptr;
    int rc = h->mem.alloc(&p, snap_stride(h) * SNAP_SLAB);
    if (rc) return rc;
    h->snap_slabs.push_back(p);
  }
  double *dst = snap_entry(h, h->n_snap);
  // same stream as the kernels: ordered after everything that wrote the committed state and before whatever
  // overwrites it; the host does not wait
  MVBA_HIP(hipMemcpyAsync(dst, h->d_X[h->cur], sizeof(double) * 3 * h->N, hipMemcpyDeviceToDevice, h->stream));
  MVBA_HIP(hipMemcpyAsync(dst + 3 * h->N, h->d_cam15[h->cur], sizeof(double) * CAM_IN * h->m, hipMemcpyDeviceToDevice, h->stream));
  h->n_snap++;
  return MVBA_OK;
}

int mvba_snapshot_count(mvba_handle *h, int64_t *n) {
  if (!h || !n) return fail(MVBA_ERR_BADARG, "null argument");
  *n = h->n_snap;
  return MVBA_OK;
}

int mvba_snapshot_read(mvba_handle *h, int64_t i, double *X, double *f, double *u, double *t, double *R) {
  if (!h || !X || !f || !u || !t || !R) return fail(MVBA_ERR_BADARG, "null argument");
  if (i < 0 || i >= h->n_snap) return fail(MVBA_ERR_BADARG, "no such log entry");
  MVBA_HIP(hipSetDevice(h->device));
  const double *src = snap_entry(h, i);
  std::vector<double> cam((size_t)h->m * CAM_IN);
  MVBA_HIP(hipMemcpyAsync(X, src, sizeof(double) * 3 * h->N, hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipMemcpyAsync(cam.data(), src + 3 * h->N, sizeof(double) * cam.size(), hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipStreamSynchronize(h->stream));
  unpack_cam15(cam.data(), h->m, f, u, t, R);
  return MVBA_OK;
}

int mvba_snapshot_restore(mvba_handle *h, int64_t i) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  if (i < 0 || i >= h->n_snap) return fail(MVBA_ERR_BADARG, "no such log entry");
  MVBA_HIP(hipSetDevice(h->device));
  const double *src = snap_entry(h, i);
  // what mvba_set_params does, from device memory: the committed state is replaced, linearisation and trial are void
  MVBA_HIP(hipMemcpyAsync(h->d_X[h->cur], src, sizeof(double) * 3 * h->N, hipMemcpyDeviceToDevice, h->stream));
  MVBA_HIP(hipMemcpyAsync(h->d_cam15[h->cur], src + 3 * h->N, sizeof(double) * CAM_IN * h->m, hipMemcpyDeviceToDevice, h->stream));
  h->have_params = true; h->linearized = false; h->have_trial = false;
  return MVBA_OK;
}

int mvba_snapshot_clear(mvba_handle *h) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  h->n_snap = 0;  // (the slabs stay for the next run; mvba_destroy frees them)
  return MVBA_OK;
}

int mvba_set_profiling(mvba_handle *h, int32_t enabled) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  h->profiling = enabled == 2 ? 2 : (enabled != 0);
  return MVBA_OK;
}

int mvba_get_stats(mvba_handle *h, mvba_stats *out) {
  if (!h || !out) return fail(MVBA_ERR_BADARG, "null argument");
  MVBA_HIP(hipSetDevice(h->device));
  int rc = sync_and_drain(h);
  if (rc) return rc;
  *out = h->stats;
  return MVBA_OK;
}

int mvba_get_info(mvba_handle *h, int64_t *out8) {
  if (!h || !out8) return fail(MVBA_ERR_BADARG, "null argument");
  out8[0] = h->n_items;
  out8[1] = h->n_items_offdiag;
  out8[2] = h->n_units;
  // bits 8..15: the slot form's step width; bit 16: the engine linearises into the compact record; bits 32..: the dense form's workgroups
  out8[3] = h->schur_mode | (h->schur_mode == SCHUR_SLOTS ? h->slot_w << 8 : 0) | (h->rec_compact ? 1 << 16 : 0) |
            (h->schur_mode == SCHUR_DENSE ? (int64_t)h->dense_blocks << 32 : 0);
  out8[4] = h->rccl_version;
  out8[5] = NCCL_VERSION_CODE;
  out8[6] = h->nranks;
  out8[7] = h->schur_mode == SCHUR_SLOTS ? h->n_slot_items : 0;  // step-major rows incl. padding
  return MVBA_OK;
}

int mvba_reset_stats(mvba_handle *h) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  MVBA_HIP(hipSetDevice(h->device));
  int rc = sync_and_drain(h);
  if (rc) return rc;
  h->stats = mvba_stats{};
  return MVBA_OK;
}

int mvba_comm_unique_id(void *id128) {
  if (!id128) return fail(MVBA_ERR_BADARG, "null argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  if (int rc = rccl_load()) return rc;
  ncclUniqueId id;
  ncclResult_t r = g_rccl.GetUniqueId(&id);
  if (r != ncclSuccess) return fail(MVBA_ERR_RCCL, std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r));
  memcpy(id128, &id, 128);
  return MVBA_OK;
}

int mvba_comm_init(mvba_handle *h, const void *id128, int32_t rank, int32_t n_ranks) {
  if (!h || !id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(MVBA_ERR_BADARG, "bad comm arguments");
  MVBA_HIP(hipSetDevice(h->device));
  if (int rc = rccl_load()) return rc;
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  ncclResult_t r = g_rccl.CommInitRank(&h->comm, n_ranks, id, rank);
  if (r != ncclSuccess) return fail(MVBA_ERR_RCCL, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r));
  h->rank = rank; h->nranks = n_ranks;
  h->rccl_version = g_rccl.version;
  int rc = h->mem.alloc(&h->d_allcost, 2 * (size_t)n_ranks);
  if (rc) return rc;
  MVBA_HIP(hipHostMalloc((void **)&h->h_allcost, 2 * sizeof(double) * n_ranks));
  return MVBA_OK;
}

int mvba_comm_init_host(mvba_handle *h, int32_t rank, int32_t n_ranks, mvba_host_allreduce_fn fn, void *user) {
  if (!h || !fn || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(MVBA_ERR_BADARG, "bad comm arguments");
  if (h->comm) return fail(MVBA_ERR_STATE, "handle already has an RCCL communicator");
  h->host_ar = fn; h->host_ar_user = user;
  h->rank = rank; h->nranks = n_ranks;
  return MVBA_OK;
}

int mvba_debug_read(mvba_handle *h, int32_t which, double *out, int64_t capacity, int64_t *n) {
  if (!h || !n) return fail(MVBA_ERR_BADARG, "null argument");
  MVBA_HIP(hipSetDevice(h->device));
  const size_t n9 = 9 * (size_t)h->m;
  long long cnt = 0;
  switch (which) {
    case MVBA_BUF_RESIDUAL: cnt = 2 * h->nobs; break;
    case MVBA_BUF_JX: cnt = 6 * h->nobs; break;
    case MVBA_BUF_JC: cnt = 18 * h->nobs; break;
    case MVBA_BUF_E: cnt = 6 * h->N; break;
    case MVBA_BUF_DP: cnt = 3 * h->N; break;
    case MVBA_BUF_A_FULL: cnt = n9 * n9; break;
    case MVBA_BUF_B_FULL: cnt = n9; break;
    case MVBA_BUF_DXI: cnt = n9; break;
    case MVBA_BUF_DX: case MVBA_BUF_TRIAL_X: cnt = 3 * h->N; break;
    case MVBA_BUF_TRIAL_CAM: cnt = (long long)CAM_IN * h->m; break;
    case MVBA_BUF_INDEX_K: case MVBA_BUF_INDEX_L: case MVBA_BUF_INDEX_A:
      cnt = h->schur_mode == SCHUR_SLOTS ? h->n_slot_items : (h->schur_mode == SCHUR_PAIRS ? h->n_items : 0);
      break;
    case MVBA_BUF_INDEX_SEG: cnt = h->schur_mode == SCHUR_SLOTS ? (long long)h->n_waves * h->slot_nseg : 0; break;
    case MVBA_BUF_WEIGHT: cnt = h->nobs; break;
    default: return fail(MVBA_ERR_BADARG, "unknown buffer id");
  }
  *n = cnt;
  if (!out) return MVBA_OK;
  if (capacity < cnt) return fail(MVBA_ERR_BADARG, "output buffer too small");
  MVBA_HIP(hipStreamSynchronize(h->stream));
  auto d2h = [&](const void *src, size_t bytes) { return hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost); };
  if (which == MVBA_BUF_RESIDUAL || which == MVBA_BUF_JX || which == MVBA_BUF_JC) {
    std::vector<double> r((size_t)2 * REC * h->nobs);  // expand the records on the host
    if (h->rec_compact) {  // ... from the compact ones, the residuals, the committed points and centres (where K1 linearised)
      const size_t no = (size_t)h->nobs;
      std::vector<double> c8(2 * REC_C * no), e2(2 * no), X(3 * (size_t)h->N), cam((size_t)CAM_IN * h->m);
      std::vector<int> pt(no), ck(no);
      MVBA_HIP(hipMemcpy(c8.data(), h->d_rec, sizeof(double) * c8.size(), hipMemcpyDeviceToHost));
      MVBA_HIP(hipMemcpy(e2.data(), h->d_res, sizeof(double) * e2.size(), hipMemcpyDeviceToHost));
      MVBA_HIP(hipMemcpy(X.data(), h->d_X[h->cur], sizeof(double) * X.size(), hipMemcpyDeviceToHost));
      MVBA_HIP(hipMemcpy(cam.data(), h->d_cam15[h->cur], sizeof(double) * cam.size(), hipMemcpyDeviceToHost));
      MVBA_HIP(hipMemcpy(pt.data(), h->d_obs_pt, sizeof(int) * no, hipMemcpyDeviceToHost));
      MVBA_HIP(hipMemcpy(ck.data(), h->d_cam, sizeof(int) * no, hipMemcpyDeviceToHost));
      for (size_t o = 0; o < no; ++o)
        expand_compact_record(&c8[2 * REC_C * o], &e2[2 * o], &X[3 * (size_t)pt[o]], &cam[(size_t)CAM_IN * ck[o] + 3], &r[2 * REC * o]);
    } else
    MVBA_HIP(hipMemcpy(r.data(), h->d_rec, sizeof(double) * r.size(), hipMemcpyDeviceToHost));
    std::vector<double> sw;  // a robust loss: the implied (u, v) columns are sqrt(w) / f0, as the Schur kernels take them
    if (h->loss != LOSS_SQUARED && which == MVBA_BUF_JC) {
      sw.resize(h->nobs);
      MVBA_HIP(hipMemcpy(sw.data(), h->d_sqw, sizeof(double) * sw.size(), hipMemcpyDeviceToHost));
    }
    for (long long o = 0; o < h->nobs; ++o) {
      const double cu = sw.empty() ? 1.0 / h->f0 : sw[o] / h->f0;
      const double *q = r.data() + (size_t)o * 2 * REC;  // slot s -> (q[2s], q[2s+1]) = (row0, row1)
      if (which == MVBA_BUF_RESIDUAL) {
        out[2 * o] = q[14]; out[2 * o + 1] = q[15];
      } else if (which == MVBA_BUF_JX) {
        for (int rr = 0; rr < 2; ++rr) for (int i = 0; i < 3; ++i) out[6 * o + 3 * rr + i] = q[2 * i + rr];
      } else {
        double *jc = out + 18 * o;
        for (int rr = 0; rr < 2; ++rr) {
          jc[9 * rr + 0] = q[6 + rr];
          jc[9 * rr + 1] = rr == 0 ? cu : 0.0;
          jc[9 * rr + 2] = rr == 1 ? cu : 0.0;
          for (int i = 0; i < 3; ++i) jc[9 * rr + 3 + i] = -q[2 * i + rr];
          for (int i = 0; i < 3; ++i) jc[9 * rr + 6 + i] = q[8 + 2 * i + rr];
        }
      }
    }
  } else if (which == MVBA_BUF_WEIGHT) {
    if (h->loss != LOSS_SQUARED) MVBA_HIP(d2h(h->d_sqw, sizeof(double) * h->nobs));
    else for (long long o = 0; o < h->nobs; ++o) out[o] = 1.0;
  } else if (which == MVBA_BUF_E || which == MVBA_BUF_DP) {
    std::vector<double> pl(9 * (size_t)h->N);
    MVBA_HIP(hipMemcpy(pl.data(), h->d_PL, sizeof(double) * pl.size(), hipMemcpyDeviceToHost));
    for (long long a = 0; a < h->N; ++a) {
      if (which == MVBA_BUF_E) for (int i = 0; i < 6; ++i) out[6 * a + i] = pl[9 * a + i];
      else for (int i = 0; i < 3; ++i) out[3 * a + i] = pl[9 * a + 6 + i];
    }
  } else if (which == MVBA_BUF_A_FULL) {  // expand the packed strips to the dense symmetric matrix
    const int m = h->m;
    std::vector<double> pk(strip_offset(m, m));
    MVBA_HIP(hipMemcpy(pk.data(), h->d_Ab, sizeof(double) * pk.size(), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < n9; ++r)
      for (size_t cc = 0; cc < n9; ++cc) {
        const size_t lo = std::min(r, cc), hi = std::max(r, cc);
        const int k = (int)(lo / 9), l = (int)(hi / 9);
        // inside a diagonal block both halves are stored: keep the entry as computed
        const size_t rr = (k == l) ? r : lo, c2 = (k == l) ? cc : hi;
        out[r * n9 + cc] = pk[strip_offset(k, m) + (rr - 9 * k) * (size_t)(9 * (m - k)) + (c2 - 9 * k)];
      }
  } else if (which == MVBA_BUF_B_FULL) {
    MVBA_HIP(d2h(h->d_Ab + strip_offset(h->m, h->m), sizeof(double) * cnt));
  } else if (which == MVBA_BUF_DXI) {
    MVBA_HIP(d2h(h->d_dxi, sizeof(double) * cnt));
  } else if (which == MVBA_BUF_DX) {
    MVBA_HIP(d2h(h->d_dX, sizeof(double) * cnt));
  } else if (which == MVBA_BUF_TRIAL_X) {
    MVBA_HIP(d2h(h->d_X[1 - h->cur], sizeof(double) * cnt));
  } else if (which == MVBA_BUF_TRIAL_CAM) {
    MVBA_HIP(d2h(h->d_cam15[1 - h->cur], sizeof(double) * cnt));
  } else if (which >= MVBA_BUF_INDEX_K && which <= MVBA_BUF_INDEX_SEG) {  // the Schur index as the kernel reads it (ints, widened)
    if (h->schur_mode == SCHUR_SLOTS && which != MVBA_BUF_INDEX_SEG) {  // one row per step: k[W] | l[W] | a[W] | pad
      const int W = h->slot_w, row = slot_idx_ints(W);
      const long long n_steps = cnt / W;
      std::vector<int> tmp((size_t)n_steps * row);
      if (cnt) MVBA_HIP(hipMemcpy(tmp.data(), h->d_it_x, sizeof(int) * tmp.size(), hipMemcpyDeviceToHost));
      const int off = which == MVBA_BUF_INDEX_K ? 0 : (which == MVBA_BUF_INDEX_L ? W : 2 * W);
      for (long long st = 0; st < n_steps; ++st)
        for (int sl = 0; sl < W; ++sl) out[st * W + sl] = (double)tmp[(size_t)st * row + off + sl];
      return MVBA_OK;
    }
    const int *src = which == MVBA_BUF_INDEX_K ? h->d_it_k : (which == MVBA_BUF_INDEX_L ? h->d_it_l : (which == MVBA_BUF_INDEX_A ? h->d_it_a : h->d_seg_end));
    std::vector<int> tmp((size_t)cnt);
    if (cnt) MVBA_HIP(hipMemcpy(tmp.data(), src, sizeof(int) * tmp.size(), hipMemcpyDeviceToHost));
    for (long long i = 0; i < cnt; ++i) out[i] = (double)tmp[i];
  }
  return MVBA_OK;
}

int mvba_project(const double *X, int64_t n_points, const double *K, const double *R, const double *t, int32_t n_images,
                 const int64_t *pt_ptr, const int32_t *cam_idx, int64_t n_obs, double *xy, int32_t device) {
  if (!X || !K || !R || !t || !xy) return fail(MVBA_ERR_BADARG, "null argument");
  if (n_points < 0 || n_images < 1 || n_obs < 0 || (pt_ptr && !cam_idx)) return fail(MVBA_ERR_BADARG, "bad sizes");
  if (!pt_ptr && n_obs != n_points * (int64_t)n_images) return fail(MVBA_ERR_BADARG, "dense grid needs n_obs = n_points * n_images");
  if (n_points >= (1LL << 31)) return fail(MVBA_ERR_BADARG, "n_points must be < 2^31");
  if ((size_t)n_images * 12 * sizeof(double) > 160 * 1024 - 256) return fail(MVBA_ERR_BADARG, "too many cameras for the LDS camera table (max 1704)");
  if (n_obs == 0) return MVBA_OK;
  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  std::vector<int> obs_pt;
  if (pt_ptr) {
    if (pt_ptr[0] != 0 || pt_ptr[n_points] != n_obs) return fail(MVBA_ERR_BADARG, "pt_ptr does not span n_obs");
    obs_pt.resize(n_obs);
    for (int64_t a = 0; a < n_points; ++a)
      for (int64_t o = pt_ptr[a]; o < pt_ptr[a + 1]; ++o) {
        if (cam_idx[o] < 0 || cam_idx[o] >= n_images) return fail(MVBA_ERR_BADARG, "cam_idx out of range");
        obs_pt[o] = (int)a;
      }
  }
  double *dX = nullptr, *dK = nullptr, *dR = nullptr, *dt = nullptr;
  double2 *dxy = nullptr;
  int *dpt = nullptr, *dcam = nullptr;
  DevBufs tmp;  // (freed on every return)
#define PRJ(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(MVBA_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
  PRJ(hipMalloc((void **)&dX, sizeof(double) * 3 * std::max<int64_t>(n_points, 1))); tmp.own(dX);
  PRJ(hipMalloc((void **)&dK, sizeof(double) * 9 * n_images)); tmp.own(dK);
  PRJ(hipMalloc((void **)&dR, sizeof(double) * 9 * n_images)); tmp.own(dR);
  PRJ(hipMalloc((void **)&dt, sizeof(double) * 3 * n_images)); tmp.own(dt);
  PRJ(hipMalloc((void **)&dxy, sizeof(double2) * n_obs)); tmp.own(dxy);
  PRJ(hipMemcpy(dX, X, sizeof(double) * 3 * n_points, hipMemcpyHostToDevice));
  PRJ(hipMemcpy(dK, K, sizeof(double) * 9 * n_images, hipMemcpyHostToDevice));
  PRJ(hipMemcpy(dR, R, sizeof(double) * 9 * n_images, hipMemcpyHostToDevice));
  PRJ(hipMemcpy(dt, t, sizeof(double) * 3 * n_images, hipMemcpyHostToDevice));
  if (pt_ptr) {
    PRJ(hipMalloc((void **)&dpt, sizeof(int) * n_obs)); tmp.own(dpt);
    PRJ(hipMalloc((void **)&dcam, sizeof(int) * n_obs)); tmp.own(dcam);
    PRJ(hipMemcpy(dpt, obs_pt.data(), sizeof(int) * n_obs, hipMemcpyHostToDevice));
    PRJ(hipMemcpy(dcam, cam_idx, sizeof(int) * n_obs, hipMemcpyHostToDevice));
  }
  const int lds = (int)(sizeof(double) * 12 * n_images);
  PRJ(hipFuncSetAttribute((const void *)k_project_obs, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_obs + 255) / 256));
  hipLaunchKernelGGL(k_project_obs, dim3(grid), dim3(256), lds, 0, (long long)n_obs, n_images, dX, dK, dR, dt, dpt, dcam, dxy);
  PRJ(hipGetLastError());
  PRJ(hipMemcpy(xy, dxy, sizeof(double2) * n_obs, hipMemcpyDeviceToHost));
#undef PRJ
  return MVBA_OK;
}

int mvba_host_obs_math(const double *X3, const double *cam15, const double *xy2, double f0, double *out26) {
  if (!X3 || !cam15 || !xy2 || !out26) return fail(MVBA_ERR_BADARG, "null argument");
  alignas(16) double c[CAM_LDS];
  expand_cam(cam15, f0, c);
  ObsJ J;
  obs_math(X3[0], X3[1], X3[2], c, xy2[0], xy2[1], f0, J);
  out26[0] = J.e0; out26[1] = J.e1;
  for (int r = 0; r < 2; ++r) for (int i = 0; i < 3; ++i) out26[2 + 3 * r + i] = J.jx[r][i];
  for (int r = 0; r < 2; ++r) for (int i = 0; i < 9; ++i) out26[8 + 9 * r + i] = J.jc[r][i];
  return MVBA_OK;
}

}  // extern "C"

#include "mvba_start.h"  // what the three headers below share: the Jacobi, the chunk tree, list checks and upload
#include "mvba_init.h"  // initial estimates: mvba_triangulate, mvba_triangulate_state, mvba_resect
#include "mvba_twoview.h"  // two-view start: mvba_covisibility, mvba_two_view
#include "mvba_ransac.h"  // robust two-view start: mvba_two_view_robust, mvba_ransac_sample
#include "mvba_homography.h"  // planar scenes: mvba_homography_robust, mvba_homography_sample
#include "mvba_resect_ransac.h"  // robust resection: mvba_resect_robust, mvba_resect_sample
#include "mvba_pose_ransac.h"    // calibrated robust resection: mvba_pose_robust, mvba_pose_refine, mvba_pose_sample
#include "mvba_tri_ransac.h"     // robust triangulation: mvba_triangulate_robust, mvba_triangulate_sample
#include "mvba_align.h"          // similarity alignment: mvba_align_robust, mvba_align, mvba_align_sample
#include "mvba_tracks.h"         // feature tracks from pairwise matches: mvba_build_tracks
#include "mvba_match.h"          // the matches themselves, from uint8 descriptors: mvba_match_descriptors
