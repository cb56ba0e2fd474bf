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
#include "mvba_engine_host.h"  // the engine's host logic without a HIP call: maps, the solve check, debug expansions, width rules

namespace mvba {
thread_local std::string g_err;
}
using namespace mvba;

#include "mvba_rccl.h"  // the RCCL binding: g_rccl, rccl_load()

// ------------------------------------------------------------------ device code, one header per stage
namespace {

#include "mvba_device.h"     // what the stages share: fixed-order sums, the camera table in LDS, REC / PBS
#include "mvba_linearize.h"  // K1 (+ K2), K3a: k_resid_jac, k_sum_split, k_point_inv
#include "mvba_schur.h"      // K3, the gather forms: k_schur_pairs*, k_schur_slots, k_schur_lanes (mvba_lanes.h), k_schur_reduce
#include "mvba_dense.h"      // K3, full visibility: k_schur_dense, k_schur_dense_finish
#include "mvba_solve.h"  // K4, device side: gauge strip, blocked Cholesky, the two back-substitutions, the pivoted-LU rescue
#include "mvba_tail.h"       // K5, K6 and the state kernels: k_backsub, k_cost, k_update_cams, k_cam_tables, k_residuals, ...
#include "mvba_index.h"      // the Schur index on the device: k_idx_*
#include "mvba_cov.h"  // marginal covariances (mvba_covariance): S^-1 from the Cholesky factor and the point pass
#include "mvba_map.h"  // parameter maps (mvba_set_parameter_map): the mapped gather into K4 and the way back

}  // namespace

// ------------------------------------------------------------------ host side, one header per concern
#include "mvba_engine.h"  // mvba_handle, the event timers, the cost mailbox, the kernel tables and LDS formulas, CreateKnobs
namespace {
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

int mvba_set_params(mvba_handle *h, const double *X, const double *f, const double *u, const double *t, const double *R) {
  if (!h || !X || !f || !u || !t || !R) return fail(MVBA_ERR_BADARG, "null argument");
  MVBA_HIP(hipSetDevice(h->device));
  std::vector<double> cam((size_t)h->m * CAM_IN);
  pack_cam15(h->m, f, u, t, R, cam.data());
  return write_state(h, X, cam.data(), hipMemcpyHostToDevice);
}

int mvba_get_params(mvba_handle *h, double *X, double *f, double *u, double *t, double *R) {
  if (!h || !X || !f || !u || !t || !R) return fail(MVBA_ERR_BADARG, "null argument");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set");
  MVBA_HIP(hipSetDevice(h->device));
  return read_state(h, h->d_X[h->cur], h->d_cam15[h->cur], X, f, u, t, R);
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

int mvba_set_parameter_map(mvba_handle *h, const int32_t *col, int32_t n_free) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  MVBA_HIP(hipSetDevice(h->device));
  const int n9 = 9 * h->m;
  if (!col) {  // the default map: the seven gauge slots held, everything else free
    h->mapped = false;
    h->have_trial = false;
    return MVBA_OK;
  }
  ParameterMap map;  // the checks and the tables: mvba_engine_host.h
  if (int rc = build_parameter_map(col, h->m, h->gauge_axis, n_free, h->D, map)) return rc;
  h->have_trial = false;
  if (map.is_default) {  // spelled out: the engine runs exactly what it runs without a map
    h->mapped = false;
    return MVBA_OK;
  }
  const std::vector<int2> &pairs = map.pairs;
  int2 *d_pairs = nullptr;
  double *d_part = nullptr;
  if (!pairs.empty()) {
    int rc = h->mem.alloc(&d_pairs, pairs.size());
    if (!rc) rc = h->mem.alloc(&d_part, pairs.size() * (size_t)map.nblk);
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
  h->map_nblk = map.nblk;
  if (!pairs.empty()) MVBA_HIP(hipMemcpy(h->d_map_pairs, pairs.data(), sizeof(int2) * pairs.size(), hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(h->d_map_col, col, sizeof(int) * n9, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(h->d_map_ptr, map.ptr.data(), sizeof(int) * (n_free + 1), hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(h->d_map_mem, map.mem.data(), sizeof(int) * map.mem.size(), hipMemcpyHostToDevice));
  h->map_col.assign(col, col + n9);
  h->map_ptr = map.ptr;
  h->map_mem = map.mem;
  h->n_free = n_free;
  h->map_ld = (n_free + 3) & ~3;
  h->map_U = map.U;
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
  MVBA_HIP(hipMalloc((void **)&dX, sizeof(double) * 3 * std::max<int64_t>(n_points, 1))); tmp.own(dX);
  MVBA_HIP(hipMalloc((void **)&dK, sizeof(double) * 9 * n_images)); tmp.own(dK);
  MVBA_HIP(hipMalloc((void **)&dR, sizeof(double) * 9 * n_images)); tmp.own(dR);
  MVBA_HIP(hipMalloc((void **)&dt, sizeof(double) * 3 * n_images)); tmp.own(dt);
  MVBA_HIP(hipMalloc((void **)&dxy, sizeof(double2) * n_obs)); tmp.own(dxy);
  MVBA_HIP(hipMemcpy(dX, X, sizeof(double) * 3 * n_points, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dK, K, sizeof(double) * 9 * n_images, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dR, R, sizeof(double) * 9 * n_images, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dt, t, sizeof(double) * 3 * n_images, hipMemcpyHostToDevice));
  if (pt_ptr) {
    MVBA_HIP(hipMalloc((void **)&dpt, sizeof(int) * n_obs)); tmp.own(dpt);
    MVBA_HIP(hipMalloc((void **)&dcam, sizeof(int) * n_obs)); tmp.own(dcam);
    MVBA_HIP(hipMemcpy(dpt, obs_pt.data(), sizeof(int) * n_obs, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dcam, cam_idx, sizeof(int) * n_obs, hipMemcpyHostToDevice));
  }
  const int lds = (int)(sizeof(double) * 12 * n_images);
  MVBA_HIP(hipFuncSetAttribute((const void *)k_project_obs, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_obs + 255) / 256));
  hipLaunchKernelGGL(k_project_obs, dim3(grid), dim3(256), lds, 0, (long long)n_obs, n_images, dX, dK, dR, dt, dpt, dcam, dxy);
  MVBA_HIP(hipGetLastError());
  MVBA_HIP(hipMemcpy(xy, dxy, sizeof(double2) * n_obs, hipMemcpyDeviceToHost));
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

#include "mvba_step.h"      // the LM step: mvba_linearize, mvba_try_step, mvba_commit and the launches they are made of
#include "mvba_cov_host.h"  // mvba_covariance, as stages
#include "mvba_debug.h"     // the snapshot log, profiling and statistics, mvba_get_info, mvba_debug_read

#include "mvba_start.h"  // what the headers below share: the Jacobi, the chunk tree, list checks and upload, the clock and event laps of a call
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
