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

// ------------------------------------------------------------------ device helpers
namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0 holds the sum; fixed tree -> deterministic
}

// Deterministic block sum (fixed tree); result valid in thread 0.
__device__ __forceinline__ double block_sum(double v, double *s_red /*[16]*/) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) s_red[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int i = 0; i < nw; ++i) t += s_red[i];
  }
  return t;
}

__device__ __forceinline__ void load_cams_to_lds(const double *__restrict__ cam15, int m, double f0,
                                                 double *s_cam) {
  for (int k = threadIdx.x; k < m; k += blockDim.x) expand_cam(cam15 + (size_t)k * CAM_IN, f0, s_cam + k * CAM_LDS);
}

// Reduced system storage: the upper block triangle of A packed strip by strip -- strip k is a
// row-major 9 x 9(m-k) block (cameras l >= k) at offset 81 (k m - k (k-1) / 2) -- followed by b
// (9m).  81 m (m+1) / 2 + 9m doubles: half of the dense 9m x 9m, and what the all-reduce ships.
__host__ __device__ __forceinline__ size_t strip_offset(int k, int m) {
  return 81 * ((size_t)k * m - (size_t)k * (k - 1) / 2);
}

__device__ __forceinline__ int keep_index(int i, int gauge_axis) {
  // i-th kept parameter -> global parameter index; removed = {3..8, 12+axis} (ref :62-72)
  if (i < 3) return i;
  return (i + 6 < 12 + gauge_axis) ? i + 6 : i + 7;
}

// Wave-uniform operands are read through the constant address space so that the compiler issues scalar (SMEM)
// loads into SGPRs instead of 64 identical vector loads.
#define MVBA_CONST_AS __attribute__((address_space(4)))
template <typename T>
__device__ __forceinline__ const T MVBA_CONST_AS *as_const(const T *p) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
  return (const T MVBA_CONST_AS *)p;
#pragma clang diagnostic pop
}

// ------------------------------------------------------------------ K1
// One thread per observation, grid-stride over 256-observation tiles; camera table
// staged once per block.  Each wave transposes its 64 records through LDS so that
// every global store instruction writes 1 KiB contiguous (8 whole lines).
// K2 is fused in: the per-point blocks E_a = 2 sum Jx^T Jx (6 unique) and dP_a = 2 sum Jx^T e
// (ref :429-469, :519-556) are formed by a wave-level segmented sum over the (point-sorted)
// observations -- PL[a][9] = Exx,Exy,Exz,Eyy,Eyz,Ezz,dP0..2 -- so the records are not re-read.
// Algorithmic traffic: 24 B in + 128 B out per observation + (24 in + 72 out) B per point.
constexpr int REC = 8;  // double2 slots per observation record (128 B)
constexpr int LDS_CAMERAS = 646;  // cameras whose tables (K1: 18 doubles + the waves' staging tiles; K5: 28 doubles) fit one workgroup's LDS

// GCAM: beyond LDS_CAMERAS cameras the expanded camera table does not fit a workgroup's LDS next to its staging tiles; the
// kernels then read the rows of a table in device memory (k_cam_tables; 144 bytes per camera, L2-resident) through the same
// 16-byte loads.  One template parameter per kernel: the LDS form keeps its ds_read_b128, nothing is decided per access.
// LOSS: a robust loss scales the observation's Jacobian rows and residual by sqrt(w) before they are stored
// and summed -- the records, E_a and dP_a are then those of the weighted least-squares problem -- and writes sqrt(w) to `sqw`.
#define MVBA_RESID_JAC_ARGS                                                                                                 \
  long long nobs, int m, const double *__restrict__ cam15, const double *__restrict__ X, const int *__restrict__ obs_pt,   \
      const int *__restrict__ cam_idx, const double2 *__restrict__ xy, double f0, const int *__restrict__ tile_start,     \
      int n_tiles, double2 *__restrict__ rec, double *__restrict__ PL, const int *__restrict__ tile_slot,                 \
      double *__restrict__ PLsplit, const double *__restrict__ gcam
// Robust kernels take one trailing argument of this type (the squared instantiations none: their arguments and code are those of
// the plain kernels).  b = (delta / f0)^2, sqw = sqrt(w) per observation.
struct LossArgs {
  double b;
  double *sqw;
};
template <bool GCAM, int LOSS = LOSS_SQUARED, typename... Robust>
__global__ __launch_bounds__(1024, 4) void k_resid_jac(MVBA_RESID_JAC_ARGS, Robust... robust) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *s_cam = smem;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  // per-wave 8 KiB staging tile, 16-byte aligned behind the camera table
  double2 *stage = reinterpret_cast<double2 *>(smem + (GCAM ? 0 : ((m * CAM_LDS + 1) & ~1))) + wave * (64 * REC);
  // the same 8 KiB is reused for the per-point sums: contrib[9][CS] doubles (odd stride: the nine
  // components of one observation sit in nine different banks), then seg_start[65], pt[64]
  constexpr int CS = 65;
  double *contrib = reinterpret_cast<double *>(stage);
  int *seg_start = reinterpret_cast<int *>(contrib + 9 * CS), *seg_pt = seg_start + 66;
  if (!GCAM) {
    load_cams_to_lds(cam15, m, f0, s_cam);
    __syncthreads();
  }
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
      obs_math(Xa[0], Xa[1], Xa[2], GCAM ? gcam + (size_t)k * CAM_LDS : s_cam + k * CAM_LDS, z.x, z.y, f0, J);
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
      // swizzled slot position (s ^ (lane & 7)): conflict-free ds_write_b128
      double2 *row = stage + lane * REC;
      const int sw = lane & 7;
      row[0 ^ sw] = make_double2(J.jx[0][0], J.jx[1][0]);
      row[1 ^ sw] = make_double2(J.jx[0][1], J.jx[1][1]);
      row[2 ^ sw] = make_double2(J.jx[0][2], J.jx[1][2]);
      row[3 ^ sw] = make_double2(J.jc[0][0], J.jc[1][0]);
      row[4 ^ sw] = make_double2(J.jc[0][6], J.jc[1][6]);
      row[5 ^ sw] = make_double2(J.jc[0][7], J.jc[1][7]);
      row[6 ^ sw] = make_double2(J.jc[0][8], J.jc[1][8]);
      row[7 ^ sw] = make_double2(J.e0, J.e1);
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
    for (int q = 0; q < REC; ++q) {
      const int ol = q * 8 + (lane >> 3), pos = lane & 7;  // local observation, stored position
      const double2 v = stage[ol * REC + pos];
      if (ol < n) rec[(wbase + ol) * REC + (pos ^ (ol & 7))] = v;
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
constexpr int PBS = 16;
constexpr int PACE_STRIDE = 32;  // ints between two pacing counters: one 128-byte line each (they are hammered by ~300 waves)
// Also clears the packed [A|b] the Schur kernel is about to accumulate into (one launch less on
// the path; the grid is sized for whichever of the two jobs is larger).
// Held points (mvba_set_point_hold): the instantiation with one trailing `const uint8_t *held` [npts] writes the
// row of a point removed from the unknowns -- E^-1 = 0, v = 0, R = 0, the tenth double 1 (a point, sign code 0) -- and does not
// test that point's determinant.  Without a mask the engine launches k_point_inv<>, whose arguments and body are the kernel's
// as it was before there were masks.
template <typename... Held>
__global__ __launch_bounds__(256) void k_point_inv(long long npts, double c, const double *__restrict__ PL,
                                                   double *__restrict__ PB, int *__restrict__ flag,
                                                   double *__restrict__ Ab, long long nAb, int *__restrict__ prog, long long nprog, int want_r,
                                                   Held... held) {
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
    }
  }
  __syncthreads();
  double2 *dst = reinterpret_cast<double2 *>(PB + PBS * a0);
  for (int e = threadIdx.x; e < 8 * np; e += 256) {
    const int p = e >> 3, sl = e & 7;
    dst[e] = s_out[8 * p + (sl ^ (p & 7))];
  }
}

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
template <int W, bool DIAG, bool PACKED>
struct SchurStage {
  static constexpr int NPS = DIAG ? 5 : 3;
  static constexpr int L = W * PROW;
  static constexpr int P = L + ((PACKED && DIAG) ? W * 16 : W * PROW);
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

// The slot form at 64 lists per wave (mvba_lanes.h): block b IS wave b / nR of range b % nR as above, its index rows are
// 768 bytes and its unit ids 64 per wave.  Not paced: no counters to clear, the pacing table of the index is not read.
__global__ __launch_bounds__(64, 1) void k_schur_lanes(const int4 *__restrict__ wdesc, const int *__restrict__ wunits,
                                                       const int *__restrict__ it_x, const double2 *__restrict__ rec,
                                                       const double *__restrict__ PB, double c, double f0,
                                                       double *__restrict__ partial, int nR,
                                                       const long long *__restrict__ range_o0) {
  extern __shared__ char smem_pairs[];
  const int bid = blockIdx.x;
  const int MVBA_CONST_AS *dp = as_const(reinterpret_cast<const int *>(wdesc)) + 4 * (size_t)bid;
  const int d_x = dp[0], d_y = dp[1], nsteps = dp[2], flags = dp[3];
  if (nsteps <= 0) return;  // (wave-uniform) a wave whose lists are all empty in this range
  const long long beg = ((long long)d_y << 32) | (unsigned)d_x;
  const int *su = wunits + (size_t)bid * LANES_W;
  const double2 *rec_r = rec + (size_t)as_const(range_o0)[bid % nR] * REC;  // record indices are relative to the range's first observation
  if (flags & 1) schur_lanes_run<true>(smem_pairs, (int)threadIdx.x, beg, nsteps, it_x, rec_r, PB, c, 1.0 / f0, partial, su);
  else schur_lanes_run<false>(smem_pairs, (int)threadIdx.x, beg, nsteps, it_x, rec_r, PB, c, 1.0 / f0, partial, su);
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

// ------------------------------------------------------------------ K3 (dense visibility: every point seen by every camera)
// The reference's own scenes (euclidiean_reconstruction.py, affine_reconstruction.py, BASELINE config 2) and the pipeline test at
// 1 M points x 12 images have FULL visibility and a dozen or two cameras.  The pair-major forms above then walk m (m + 1) / 2 items
// per point through gathers and an index of their own (78 items and 0.9 GB of index per million points at 12 cameras: 4.9 ms per
// solve, 63 ps per item against 30 at config 3) although a point's m records are ONE contiguous range and every pair is present.
// With E_a^-1 = R_a R_a^T (3 x 3 Cholesky) and the scaled camera Jacobian J~_ak (2 x 9: f | u, v (1 / f0) | t (-J_X) | omega)
//   G_a = [R_a^T J_Xak^T J~_ak]_k   (3 x 9m),        A = blockdiag(2 H_k + c diag(2 H_k)) - 4 sum_a G_a^T G_a,
//   H_k = sum_a J~_ak^T J~_ak,                        b_k = 2 sum_a J~_ak^T (J_Xak E_a^-1 dP_a - e_ak)
// -- one symmetric rank-3N update of a 9m x 9m matrix: a GEMM, on the f64 matrix cores, over records streamed ONCE.
// A workgroup takes a chunk of points (dense_ch: 4 or 8) at a time: their records and point rows go into LDS with contiguous 16-byte loads; a thread per
// observation forms J_X R and the right-hand-side vector w; the rows of G are written to LDS once (each is read by up to T tile
// pairs); wave w then owns the 16 x 16 tile pairs w, w + 4, ... of the upper triangle (four consecutive rows of G -- of whichever
// points -- are one v_mfma_f64_16x16x4: no padding of K) and the per-camera tiles [J~ | w]^T [J~ | w] (two points per MFMA) of the
// cameras w, w + 4, ...  Partial tiles per workgroup, summed in workgroup order by k_schur_dense_finish: no atomics, bitwise
// reproducible.  No index at all: mvba_create skips the pair-major index for such scenes.
typedef double mvba_d4 __attribute__((ext_vector_type(4)));
// Points per chunk (= producer waves) and workgroups per CU.  Up to 7 tiles (12 cameras) the kernel needs at most 126 registers: four
// waves fit a SIMD, so TWO 8-wave workgroups of 4-point chunks (~53 KB of LDS each) share a CU and fill each other's barrier waits
// (1.335 -> 1.260 ms at 1 M x 12, 1.48 -> 1.32 at 2 M x 6; three workgroups: worse again).  8 tiles take 154 registers -- three waves
// per SIMD -- and stay with one 12-wave workgroup of 8-point chunks (two of the small ones cannot both be resident: 1.65 -> 1.82 ms
// at 14 cameras); beyond that eight consumer + four producer waves.  (tools/dense_ch.sh, profiles/r05_dense_form.txt)
constexpr int dense_ch(int T) { return T == 8 ? 8 : 4; }
constexpr int dense_wgs(int T) { return T <= 7 ? 2 : 1; }
constexpr int DENSE_MAX_TILES = 12;  // 9 m <= 192: m <= 21 cameras (78 tile pairs: 20 accumulators of 4 doubles per lane)
__device__ __forceinline__ int dense_tile_elem(int row, int col) { return ((row >> 2) << 6) | ((row & 3) << 4) | col; }  // C/D layout: col = l & 15, row = (l >> 4) + 4 reg

constexpr int dense_pair_ti(int p, int T) { int a = 0; while (p >= T - a) { p -= T - a; ++a; } return a; }
constexpr int dense_pair_tj(int p, int T) { int a = 0; while (p >= T - a) { p -= T - a; ++a; } return a + p; }
constexpr int dense_consumers(int T) { return T <= 8 ? 4 : 8; }  // consumer waves: at most ~10 tile pairs (40 accumulator doubles) each
constexpr bool dense_tile_used(int u, int T, int wave) {  // does consumer wave `wave` own a pair with tile u?
  const int P = T * (T + 1) / 2, NC = dense_consumers(T);
  for (int p = wave; p < P; p += NC)
    if (dense_pair_ti(p, T) == u || dense_pair_tj(p, T) == u) return true;
  // (its spare slots repeat the last pair)
  return (P + NC - 1) / NC * NC - NC + wave >= P && (dense_pair_ti(P - 1, T) == u || dense_pair_tj(P - 1, T) == u);
}
// the main products of one chunk for consumer wave WAVE: its tile pairs p = NC q + WAVE are known at compile time, so the operand of a
// tile is read from LDS ONCE per four rows of G and used from its register by every pair that needs it (two reads per MFMA, with
// the tiles indexed at run time, kept the LDS half busy under the matrix cores).  (The pair -> tile arithmetic goes through class
// templates: called as constexpr FUNCTIONS inside the unrolled loops it was evaluated at run time, with the registers indexed
// through s_set_gpr_idx.)
template <int T, int WAVE, int Q>
struct DensePair {
  static constexpr int P = T * (T + 1) / 2, NC = dense_consumers(T);
  static constexpr int p = NC * Q + WAVE < P ? NC * Q + WAVE : P - 1;  // (a spare slot repeats the last pair: computed, never stored)
  static constexpr int ti = dense_pair_ti(p, T), tj = dense_pair_tj(p, T);
};
template <int T, int WAVE, int U>
struct DenseUsed { static constexpr bool v = dense_tile_used(U, T, WAVE); };
template <int T, int WAVE, int... U>
__device__ __forceinline__ void dense_load_tiles(const double *row, double (&t)[T], std::integer_sequence<int, U...>) {
  ((t[U] = DenseUsed<T, WAVE, U>::v ? row[16 * U] : 0.0), ...);
}
template <int T, int WAVE, int... Q>
__device__ __forceinline__ void dense_mfma_pairs(const double (&ts)[T], const double (&t)[T], mvba_d4 *acc, std::integer_sequence<int, Q...>) {
  ((acc[Q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ts[DensePair<T, WAVE, Q>::ti], t[DensePair<T, WAVE, Q>::tj], acc[Q], 0, 0, 0)), ...);
}
template <int T, int WAVE, int CH>
__device__ __forceinline__ void dense_main_mfma(const double *sG, const double *sSgn, int li, int lk, mvba_d4 *acc) {
  constexpr int P = T * (T + 1) / 2, NC = dense_consumers(T), NPW = (P + NC - 1) / NC, W = 16 * T;
#pragma unroll
  for (int g = 0; g < 3 * CH / 4; ++g) {  // four rows of G per MFMA: sum_r s_r g_r^T g_r (s = +-1: E^-1 = R S R^T), the sign on the left operand
    double t[T], ts[T];
    dense_load_tiles<T, WAVE>(sG + (size_t)(4 * g + lk) * W + li, t, std::make_integer_sequence<int, T>{});
    const double sg = sSgn[4 * g + lk];
#pragma unroll
    for (int u = 0; u < T; ++u) ts[u] = t[u] * sg;
    dense_mfma_pairs<T, WAVE>(ts, t, acc, std::make_integer_sequence<int, NPW>{});
  }
}

// Two roles in a workgroup, one barrier per chunk: waves 0-3 multiply chunk i (main pairs and camera tiles out of the buffers of
// parity i & 1) while the producer waves -- one per point of a chunk -- build chunk i + 1 into the other buffers, each taking its
// point from its records (fetched into registers a chunk earlier) to the rows of G on its own, so the producers need no barrier
// among themselves.  (With every wave doing every phase in turn -- four barriers per chunk -- the workgroups of a CU ran in
// lockstep and the phases never overlapped: 1.55 ms at 1 M x 12 for 0.81 ms of MFMA phase; with four producer waves of two points
// each the producers were the longer role: 1.90 ms.)
// ROBUST: the records are scaled by sqrt(w) (K1); the constant columns of an observation become sqrt(w) / f0
// instead of 1 / f0 -- the per-(point, camera) factor sF takes sqrt(w) from `sqw`, fetched with the records.
#define MVBA_DENSE_ARGS                                                                                                   \
  const double2 *__restrict__ rec, const double *__restrict__ PB, const int *__restrict__ obs_of, long long N, int m, double cu, \
      double *__restrict__ part
template <int T, bool TABLE, bool ROBUST = false, typename... Robust>  // TABLE: the records of a point through obs_of (missing observations), otherwise one contiguous range
__global__ __launch_bounds__(64 * (dense_consumers(T) + dense_ch(T))) void k_schur_dense(MVBA_DENSE_ARGS, Robust... robust) {
  constexpr int NC = dense_consumers(T);           // consumer waves (4 + 8 producers up to 8 tiles, 8 + 4 beyond)
  constexpr int P = T * (T + 1) / 2, NPW = (P + NC - 1) / NC, W = 16 * T, NCW = ((16 * T) / 9 + NC - 1) / NC;
  constexpr int CH = dense_ch(T);       // points per chunk = producer waves (the double-buffered rows must fit the LDS beside each other)
  constexpr int MMAX = (16 * T) / 9;               // cameras at most
  constexpr int NTHR = 64 * (NC + CH);
  extern __shared__ double2 dsm[];
  double *sG = reinterpret_cast<double *>(dsm);                     // [2][3 CH][W]
  double *sB = sG + (size_t)2 * 3 * CH * W;                         // [2][CH m][2][16]: rows x, y of [J~ (9) | w | 0 ...]
  double2 *sScr = reinterpret_cast<double2 *>(sB + (size_t)2 * CH * m * 32);  // per producer wave: records [m][8], point row [8]
  double *sFlag = reinterpret_cast<double *>(sScr + (size_t)CH * (m * REC + 8));  // per producer wave: [m] 1 for an observation, 0 for a missing one
  double *sSgn = sFlag + (size_t)CH * m;                            // [2][3 CH]: the signs of the rows of G
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;  // (wave through readfirstlane -- scalar address arithmetic for the producers -- made every shape slower: 1.36 -> 1.55 ms at 1 M x 12, 2.95 -> 12.6 at 20 cameras)
  const long long n_chunks = (N + CH - 1) / CH;
  // what no phase ever writes stays zero: the columns of G beyond 9 m, the columns 10..15 of the camera rows
  for (int e = threadIdx.x; e < 2 * 3 * CH * W; e += NTHR) sG[e] = 0.0;
  for (int e = threadIdx.x; e < 2 * CH * m * 32; e += NTHR) sB[e] = 0.0;
  __syncthreads();
  if (wave >= NC) {
    // ---------------- producer: point pw of every chunk of this workgroup.  (Without the staging -- a lane per (camera, column)
    // fetching its four record slots itself -- the per-lane loads cost more than the staging saves: 1.82 against 1.40 ms.)
    const int pw = wave - NC;
    // The producers are the longer role (role trace, profiles/r05_dense_form.txt: 5,350 cycles of work per chunk against the consumers' 4,480 + 1,400 at
    // the barrier, 1 M x 12) and, as the later-dispatched waves of their SIMD, the losers of its issue arbitration (older first at
    // equal priority): they ask for the higher priority once, here.
    __builtin_amdgcn_s_setprio(1);
    double2 *sR = sScr + (size_t)pw * (m * REC + 8), *sP = sR + (size_t)m * REC;
    constexpr int NPRE = (MMAX * REC + 63) / 64, NIT = (MMAX * 10 + 63) / 64;
    // TWO chunks' records in flight per wave (sets A and B, used in turn): with one, a CU had 8 waves x 1.5 KB outstanding against
    // ~2 us of loaded memory latency -- 1.5 TB/s over the chip, which is where the kernel sat at every camera count (~1.0 ms per
    // million points x 12 cameras whatever the matrix cores had to do)
    double2 preA[NPRE], prepbA, preB[NPRE], prepbB;
    double swA[NPRE], swB[NPRE];                   // ROBUST: sqrt(w) of the observation of every record slot a lane fetched
    bool lvA, lvB;
    int oidA[NPRE], oidB[NPRE], oid_next[NPRE];    // (obs_of != nullptr) the observations of a set's point / of the point fetched next
    double *sF = sFlag + (size_t)pw * m;
    auto fetch_ids = [&](long long ch) {           // the table row of chunk ch's point (one entry per record: eight lanes share it)
      const long long a = ch * CH + pw;
#pragma unroll
      for (int u = 0; u < NPRE; ++u) {
        const int e = lane + 64 * u;
        const int got = obs_of[(size_t)min(a, N - 1) * m + min(e >> 3, m - 1)], msk = (a < N && e < m * REC) ? -1 : 0;
        oid_next[u] = (got & msk) | ~msk;          // (-1 outside; the load itself is unconditional, see fetch)
      }
    };
    auto fetch = [&](long long ch, double2 (&pre)[NPRE], int (&oid)[NPRE], double2 &prepb, bool &lv, double (&sw)[NPRE]) {  // this wave's records and point row of chunk ch (zeros past the last point)
      // The loads are UNCONDITIONAL on clamped addresses and what must be zero (a missing observation, a point past the end) is
      // zeroed on the bit pattern in build(): behind a lane-dependent branch the compiler cannot count the loads in flight and
      // waits for all of them (vmcnt(0)) -- the other set's too, which is the one meant to stay in flight
      const long long a = ch * CH + pw;
      const bool live = lv = a < N;
      if (TABLE) {                                 // through the table read a chunk earlier
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
          oid[u] = oid_next[u];
          pre[u] = rec[(size_t)max(oid[u], 0) * REC + ((lane + 64 * u) & 7)];
          if constexpr (ROBUST) sw[u] = (robust, ...).sqw[max(oid[u], 0)];
        }
      } else {
        const double2 *src = rec + (size_t)min(a, N - 1) * m * REC;
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
          pre[u] = src[min(lane + 64 * u, m * REC - 1)];
          oid[u] = live ? 0 : -1;
          if constexpr (ROBUST) sw[u] = (robust, ...).sqw[(size_t)min(a, N - 1) * m + min((lane + 64 * u) >> 3, m - 1)];
        }
      }
      prepb = reinterpret_cast<const double2 *>(PB + (size_t)min(a, N - 1) * PBS)[lane & 7];
    };
    auto keep = [](bool c, double2 v) -> double2 {  // c ? v : 0 without a branch the load could sink under
      const long long msk = c ? -1LL : 0LL;
      return double2{__longlong_as_double(__double_as_longlong(v.x) & msk), __longlong_as_double(__double_as_longlong(v.y) & msk)};
    };
    auto build = [&](int buf, const double2 (&pre)[NPRE], const int (&oid)[NPRE], const double2 &prepb, bool lv, const double (&sw)[NPRE]) {  // registers -> the rows of G and the camera rows of this wave's point in buffer `buf`
#pragma unroll
      for (int u = 0; u < NPRE; ++u) {
        const int e = lane + 64 * u;
        if (e < m * REC) sR[e] = keep(oid[u] >= 0, pre[u]);
        if (e < m * REC && (e & 7) == 0) sF[e >> 3] = oid[u] >= 0 ? (ROBUST ? sw[u] : 1.0) : 0.0;
      }
      sP[lane & 7] = keep(lv, prepb);             // (every lane, eight copies of each slot: a store under `lane < 8` drew a vmcnt(0))
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      // point row: E^-1 (6) | E^-1 dP (3) | sign code | R lower triangular (r00 r10 r20 r11 r21 r22) of E^-1 = R S R^T (k_point_inv), the same for every lane
      const double *pb = reinterpret_cast<const double *>(sP);
      const double d0 = pb[6], d1 = pb[7], d2 = pb[8];
      const double r00 = pb[10], r10 = pb[11], r20 = pb[12], r11 = pb[13], r21 = pb[14], r22 = pb[15];
      double *gB = sB + ((size_t)buf * CH + pw) * m * 32;
      double *gG = sG + ((size_t)buf * 3 * CH + (size_t)3 * pw) * W;
      if (lane < 3) sSgn[(size_t)buf * 3 * CH + 3 * pw + lane] = (((int)pb[9] - 1) >> lane) & 1 ? -1.0 : 1.0;
      // a lane per (camera k, column j <= 9): column j of J~ (f | u, v (1 / f0) | t (-J_X) | omega) into the two camera rows and
      // G[r][9 k + j] = (J_X R)[:, r] . J~[:, j] (E^-1 = R R^T); j = 9: w = J_X E^-1 dP - e, the tenth column of the camera rows
#pragma unroll
      for (int u = 0; u < NIT; ++u) {
        const int e = lane + 64 * u, k = e / 10, j = e - 10 * k;
        if (e < 10 * m) {
          const double2 *r = sR + (size_t)k * REC;
          const double2 x0 = r[0], x1 = r[1], x2 = r[2];
          const double2 cv = r[j == 0 ? 3 : (j < 6 ? (j < 3 ? 0 : j - 3) : (j < 9 ? j - 2 : 7))];
          if (j == 9) {
            gB[(size_t)k * 32 + 9] = x0.x * d0 + x1.x * d1 + x2.x * d2 - cv.x;
            gB[(size_t)k * 32 + 25] = x0.y * d0 + x1.y * d1 + x2.y * d2 - cv.y;
          } else {
            const double sg = (j >= 3 && j < 6) ? -1.0 : 1.0, live = sF[k] * cu;  // (the constant columns 1 / f0 of an observation that exists)
            const double jx = j == 1 ? live : (j == 2 ? 0.0 : sg * cv.x), jy = j == 2 ? live : (j == 1 ? 0.0 : sg * cv.y);
            gB[(size_t)k * 32 + j] = jx;
            gB[(size_t)k * 32 + 16 + j] = jy;
            double *g = gG + 9 * k + j;
            g[0] = (x0.x * r00 + x1.x * r10 + x2.x * r20) * jx + (x0.y * r00 + x1.y * r10 + x2.y * r20) * jy;
            g[W] = (x1.x * r11 + x2.x * r21) * jx + (x1.y * r11 + x2.y * r21) * jy;
            g[2 * W] = (x2.x * r22) * jx + (x2.y * r22) * jy;
          }
        }
      }
    };
    long long ch = blockIdx.x;
    const long long gs = gridDim.x;
    // (a fetch past the last chunk loads nothing: zero records nobody reads; fetch_ids likewise -1)
    if (TABLE) fetch_ids(ch);
    fetch(ch, preA, oidA, prepbA, lvA, swA);
    if (TABLE) fetch_ids(ch + gs);
    fetch(ch + gs, preB, oidB, prepbB, lvB, swB);
    if (TABLE) fetch_ids(ch + 2 * gs);
    build(0, preA, oidA, prepbA, lvA, swA);
    fetch(ch + 2 * gs, preA, oidA, prepbA, lvA, swA);
    if (TABLE) fetch_ids(ch + 3 * gs);
    __syncthreads();
    // One barrier per chunk, as the consumers; the sets alternate: B holds chunk ch + 1, A chunk ch + 2.  Nothing in the body is
    // conditional (behind `if (ch + gs < n_chunks)` the compiler lost count of the loads in flight and waited vmcnt(0) for both
    // sets): past the last chunk a build writes a chunk of zeros into the buffer nobody reads any more.
    for (int b = 0; ch < n_chunks;) {
      build(b ^ 1, preB, oidB, prepbB, lvB, swB);
      fetch(ch + 3 * gs, preB, oidB, prepbB, lvB, swB);
      if (TABLE) fetch_ids(ch + 4 * gs);
      __syncthreads();
      ch += gs, b ^= 1;
      if (ch >= n_chunks) break;
      build(b ^ 1, preA, oidA, prepbA, lvA, swA);
      fetch(ch + 3 * gs, preA, oidA, prepbA, lvA, swA);
      if (TABLE) fetch_ids(ch + 4 * gs);
      __syncthreads();
      ch += gs, b ^= 1;
    }
    return;
  }
  // ---------------- consumer: tile pairs NC q + wave of the upper triangle (row-major), cameras NC q + wave
  mvba_d4 acc[NPW], cacc[NCW];
#pragma unroll
  for (int q = 0; q < NPW; ++q) acc[q] = mvba_d4{0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < NCW; ++q) cacc[q] = mvba_d4{0, 0, 0, 0};
  __syncthreads();  // chunk 0 is built
  int b = 0;
  for (long long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x, b ^= 1) {
    const double *bG = sG + (size_t)b * 3 * CH * W, *bB = sB + (size_t)b * CH * m * 32, *bS = sSgn + (size_t)b * 3 * CH;
    switch (wave) {  // (uniform)
      case 0: dense_main_mfma<T, 0, CH>(bG, bS, li, lk, acc); break;
      case 1: dense_main_mfma<T, 1, CH>(bG, bS, li, lk, acc); break;
      case 2: dense_main_mfma<T, 2, CH>(bG, bS, li, lk, acc); break;
      case 3: dense_main_mfma<T, 3, CH>(bG, bS, li, lk, acc); break;
      case 4: dense_main_mfma<T, 4 % NC, CH>(bG, bS, li, lk, acc); break;  // (cases 4..7 exist with eight consumers only)
      case 5: dense_main_mfma<T, 5 % NC, CH>(bG, bS, li, lk, acc); break;
      case 6: dense_main_mfma<T, 6 % NC, CH>(bG, bS, li, lk, acc); break;
      default: dense_main_mfma<T, 7 % NC, CH>(bG, bS, li, lk, acc); break;
    }
#pragma unroll
    for (int g = 0; g < CH / 2; ++g) {  // the per-camera tiles: rows (point 2 g, x), (2 g, y), (2 g + 1, x), (2 g + 1, y)
      const int pa = 2 * g + (lk >> 1), d = lk & 1;
#pragma unroll
      for (int q = 0; q < NCW; ++q) {
        const int k = min(NC * q + wave, m - 1);
        const double v = bB[(size_t)(pa * m + k) * 32 + 16 * d + li];
        cacc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, cacc[q], 0, 0, 0);
      }
    }
    __syncthreads();  // this chunk's buffers may be rebuilt, the next chunk's are complete
  }
  double *out = part + (size_t)blockIdx.x * (P + m) * 256;
#pragma unroll
  for (int q = 0; q < NPW; ++q) {
    const int p = NC * q + wave;
    if (p < P)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)p * 256 + r * 64 + lane] = acc[q][r];
  }
#pragma unroll
  for (int q = 0; q < NCW; ++q) {
    const int k = NC * q + wave;
    if (k < m)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)(P + k) * 256 + r * 64 + lane] = cacc[q][r];
  }
}

// One wave per element of the packed strips [A | b]: the workgroups' partial tiles summed in workgroup order (lane l takes the
// workgroups l, l + 64, ... in order, then a fixed tree).
__global__ __launch_bounds__(256) void k_schur_dense_finish(int m, int T, int blocks, const double *__restrict__ part, double c,
                                                            double *__restrict__ Afull, double *__restrict__ bfull) {
  const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, P = T * (T + 1) / 2;
  const long long nA = (long long)strip_offset(m, m);
  if (e >= nA + 9 * m) return;
  const size_t bstride = (size_t)(P + m) * 256;
  auto total = [&](int tile, int elem) {
    double t = 0.0;
    for (int b = lane; b < blocks; b += 64) t += part[(size_t)b * bstride + (size_t)tile * 256 + elem];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    return t;  // (valid in lane 0)
  };
  if (e < nA) {
    int k = 0;
    while (k + 1 < m && (long long)strip_offset(k + 1, m) <= e) ++k;
    const int Wk = 9 * (m - k), rem = (int)(e - (long long)strip_offset(k, m)), i = rem / Wk, cr = rem - i * Wk, l = k + cr / 9, j = cr - 9 * (l - k);
    const int gi = 9 * k + i, gj = 9 * l + j, lo = min(gi, gj), hi = max(gi, gj), ti = lo >> 4, tj = hi >> 4;
    double v = -4.0 * total(ti * T - ti * (ti - 1) / 2 + (tj - ti), dense_tile_elem(lo & 15, hi & 15));
    if (k == l) {
      const double hk = total(P + k, dense_tile_elem(i, j));
      v += 2.0 * hk * (i == j ? 1.0 + c : 1.0);  // G_k and its Marquardt term c diag(G_k)   (ref :123-125)
    }
    if (lane == 0) Afull[e] = v;
  } else {
    const int q = (int)(e - nA), k = q / 9, j = q - 9 * k;
    const double v = 2.0 * total(P + k, dense_tile_elem(j, 9));  // 2 Jc_k^T (Jx_k E^-1 dP - e)
    if (lane == 0) bfull[q] = v;
  }
}

#include "mvba_solve.h"  // K4, device side: gauge strip, blocked Cholesky, the two back-substitutions, the pivoted-LU rescue

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
  if (!GCAM) {
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
  load_cams_to_lds(cam15, m, f0, s_cam);
  __syncthreads();
  }
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
        obs_backsub(Xa0, Xa1, Xa2, GCAM ? gcam + (size_t)kk[u] * CAM_LDS : s_cam + kk[u] * CAM_LDS, GCAM ? gdxi + (size_t)DXI_LDS * kk[u] : s_dxi + DXI_LDS * kk[u], f0, t0, t1, t2);
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
      obs_backsub(Xa0, Xa1, Xa2, GCAM ? gcam + (size_t)k * CAM_LDS : s_cam + k * CAM_LDS, GCAM ? gdxi + (size_t)DXI_LDS * k : s_dxi + DXI_LDS * k, f0, t0, t1, t2);
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
  if (!GCAM) {
    load_cams_to_lds(cam15, m, f0, s_cam);
    __syncthreads();
  }
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
    const double so = obs_cost(X0, X1, X2, GCAM ? gcam + (size_t)k * CAM_LDS : s_cam + k * CAM_LDS, z.x, z.y, f0);
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
  if (!GCAM) {
    load_cams_to_lds(cam15, m, f0, s_cam);
    __syncthreads();
  }
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < nobs; o += (long long)gridDim.x * blockDim.x) {
    const int a = obs_pt[o], k = cam_idx[o];
    const double2 z = xy[o];
    double e0, e1;
    obs_resid(X[3 * (size_t)a], X[3 * (size_t)a + 1], X[3 * (size_t)a + 2], GCAM ? gcam + (size_t)k * CAM_LDS : s_cam + k * CAM_LDS,
              z.x, z.y, f0, e0, e1);
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

// ------------------------------------------------------------------ Schur index on the device (mvba_create)
// The slot form's index -- every (point, camera pair) item, counting-sorted by pair with ascending points inside a
// pair, dealt into sub-lists, then merged wave by wave into step-major rows -- built by kernels instead of 16 host
// threads (0.7 s of a 0.83 s mvba_create at config 3).  A STABLE counting sort: wave w owns a contiguous chunk of
// points and walks them in order, its lanes taking the items of one (point, first camera) row at a time -- distinct
// pairs, so the wave's private histogram in LDS needs no atomics and an item's rank inside its pair is
// [items of earlier waves] + [items of this wave so far]: exactly the position the host's sequential pass gives it.
constexpr int IDX_WAVES = 4;  // waves per block of the counting / filling kernels (one P-int histogram each in LDS)

__device__ __forceinline__ int idx_pair_id(int k, int l, int m) { return k * m - k * (k - 1) / 2 + (l - k); }

// hist[w][q] = items of pair q among the points of wave w's chunk.
// GLOBAL: the pair histogram does not fit LDS (more than ~138 cameras: 125 k pairs at 500) -- the wave counts in its
// own row of `hist` in device memory instead (zeroed by the caller).  Same walk, same ranks; a row visit is then a
// dependent round trip to L2 (agent-scope accesses: a later visit of the same pair, possibly from another lane of
// this wave, must see the count), ~1-2 us per (point, first camera) row instead of ~0.1.
template <bool GLOBAL>
__global__ __launch_bounds__(64 * IDX_WAVES) void k_idx_count(long long N, int m, int P, const long long *__restrict__ pt_ptr,
                                                              const int *__restrict__ cam_idx, int chunk,
                                                              int *__restrict__ hist, const int *__restrict__ order) {
  extern __shared__ int s_hist_all[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long w = (long long)blockIdx.x * IDX_WAVES + wv;
  int *s_hist = GLOBAL ? hist + (size_t)w * P : s_hist_all + (size_t)wv * P;
  if (!GLOBAL) {
    for (int q = lane; q < P; q += 64) s_hist[q] = 0;
    wave_sync();
  }
  const long long a0 = w * chunk, a1 = min(N, a0 + chunk);
  for (long long ai = a0; ai < a1; ++ai) {
    const long long a = order ? order[ai] : ai;  // (a sweep order of the points; mvba_create sweeps them in their natural order and passes none)
    const long long o0 = pt_ptr[a];
    const int d = (int)(pt_ptr[a + 1] - o0);
    for (int i = 0; i < d; ++i) {
      const int k = cam_idx[o0 + i];
      for (int j = i + lane; j < d; j += 64) {  // distinct pairs per instruction
        int *c = s_hist + idx_pair_id(k, cam_idx[o0 + j], m);
        if (GLOBAL) __hip_atomic_store(c, __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *c += 1;
      }
      wave_sync();
    }
  }
  if (!GLOBAL)
    for (int q = lane; q < P; q += 64) hist[(size_t)w * P + q] = s_hist[q];
}

// exclusive prefix over the waves, per pair (in place); cnt[q] = total
__global__ void k_idx_scan(int P, int n_waves, int *__restrict__ hist, long long *__restrict__ cnt) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P) return;
  long long run = 0;
  for (int w = 0; w < n_waves; ++w) {
    const int v = hist[(size_t)w * P + q];
    hist[(size_t)w * P + q] = (int)run;
    run += v;
  }
  cnt[q] = run;
}

// the same walk again: item r of pair q goes to sub-list r % S[q], position r / S[q] (the host's dealing)
// (GLOBAL: the running ranks live in the wave's row of `hist` itself, which the scan has turned into start ranks)
template <bool GLOBAL>
__global__ __launch_bounds__(64 * IDX_WAVES) void k_idx_fill(long long N, int m, int P, const long long *__restrict__ pt_ptr,
                                                             const int *__restrict__ cam_idx, int chunk,
                                                             int *__restrict__ hist, const int *__restrict__ S,
                                                             const int *__restrict__ vp_ptr, const long long *__restrict__ vp_off,
                                                             int *__restrict__ it_k, int *__restrict__ it_l, int *__restrict__ it_a,
                                                             const int *__restrict__ order) {
  extern __shared__ int s_hist_all[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long w = (long long)blockIdx.x * IDX_WAVES + wv;
  int *s_rank = GLOBAL ? hist + (size_t)w * P : s_hist_all + (size_t)wv * P;
  if (!GLOBAL) {
    for (int q = lane; q < P; q += 64) s_rank[q] = hist[(size_t)w * P + q];  // items of earlier waves
    wave_sync();
  }
  const long long a0 = w * chunk, a1 = min(N, a0 + chunk);
  for (long long ai = a0; ai < a1; ++ai) {
    const long long a = order ? order[ai] : ai;
    const long long o0 = pt_ptr[a];
    const int d = (int)(pt_ptr[a + 1] - o0);
    for (int i = 0; i < d; ++i) {
      const int k = cam_idx[o0 + i];
      for (int j = i + lane; j < d; j += 64) {
        const int q = idx_pair_id(k, cam_idx[o0 + j], m);
        int r;
        if (GLOBAL) {
          r = __hip_atomic_load(s_rank + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(s_rank + q, r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          r = s_rank[q];
          s_rank[q] = r + 1;
        }
        const int sq = S[q];
        const long long pos = vp_off[vp_ptr[q] + (r % sq)] + r / sq;
        it_k[pos] = (int)(o0 + i);
        it_l[pos] = (int)(o0 + j);
        it_a[pos] = (int)a;
      }
      wave_sync();
    }
  }
}

// lo[v][r] = first item of list v whose point is >= range_lo[r]  (r = 0 .. nR: the last column is the list's end)
__global__ void k_idx_bounds(int VP, int nR, const long long *__restrict__ vp_off, const long long *__restrict__ range_lo,
                             const int *__restrict__ it_a, long long *__restrict__ lo, const int *__restrict__ rank) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)VP * (nR + 1)) return;
  const int v = (int)(t / (nR + 1)), r = (int)(t - (long long)v * (nR + 1));
  long long b = vp_off[v], e = vp_off[v + 1];
  const long long key = range_lo[r];
  while (b < e) {  // lower_bound
    const long long mid = (b + e) >> 1;
    if ((rank ? rank[it_a[mid]] : it_a[mid]) < key) b = mid + 1;  // (a list is ascending in sweep order; ranges are contiguous in it)
    else e = mid;
  }
  lo[t] = b;
}

// The bounded-skew merge of one wave's W lists (W = 21: k_schur_slots, 64: k_schur_lanes), lane = slot.  FILL = false: count the
// steps.  FILL = true: write the step-major rows (record indices RELATIVE to the range's first observation), the pacing table
// (steps taken when the slowest slot leaves a segment) and the padding rows (`pad_obs` = 0: the range's first record,
// any finite one will do, times `pad_pt` = N: the all-zero point row).
template <bool FILL, int W>
__global__ __launch_bounds__(64) void k_idx_merge(long long n_waves, int nR, int nSeg, long long skew, long long segG,
                                                  const long long *__restrict__ sl_beg, const int *__restrict__ sl_len,
                                                  const long long *__restrict__ range_o0, const int *__restrict__ it_k,
                                                  const int *__restrict__ it_l, const int *__restrict__ it_a,
                                                  const long long *__restrict__ w_beg, int pad_obs, int pad_pt,
                                                  int *__restrict__ w_steps, int *__restrict__ st_k, int *__restrict__ st_l,
                                                  int *__restrict__ st_a, int *__restrict__ seg_end, const long long *__restrict__ pkey) {
  static_assert(W >= 1 && W <= 64, "one lane per slot");
  const long long b = blockIdx.x;
  const int lane = threadIdx.x;
  const bool slot = lane < W;
  long long cur = slot ? sl_beg[b * W + lane] : 0;
  const long long end = slot ? cur + sl_len[b * W + lane] : 0;
  const long long o_lo = range_o0[b % nR];
  const long long base = FILL ? w_beg[b] : 0;
  constexpr long long NONE = 1LL << 40;
  int steps = 0, sg = 0;
  // an item's key = where its point sits in the sweep, in observations (pkey[a] = observations of the points swept
  // before a; with the natural order that is a's first observation); the k-side record index is what goes into the row
  // two keys ahead in registers: the next step's key never waits for a load issued in this step
  auto key_at = [&](long long c) -> long long { return pkey[it_a[c]]; };
  long long k0 = cur < end ? key_at(cur) : NONE, k1 = cur + 1 < end ? key_at(cur + 1) : NONE;
  while (true) {
    long long lo = k0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lo = min(lo, __shfl_xor(lo, off, 64));
    if (FILL && lo < NONE && lane == 0)
      while (sg < nSeg && lo >= o_lo + (sg + 1) * segG) seg_end[b * nSeg + sg++] = steps;
    if (lo >= NONE) break;
    const bool take = k0 < NONE && k0 <= lo + skew;
    if (FILL && slot) {
      const long long o = (base + steps) * W + lane;
      st_k[o] = take ? (int)(it_k[cur] - o_lo) : pad_obs;  // record indices relative to the range's first observation
      st_l[o] = take ? (int)(it_l[cur] - o_lo) : pad_obs;
      st_a[o] = take ? it_a[cur] : pad_pt;
    }
    if (take) {
      ++cur;
      k0 = k1;
      k1 = cur + 1 < end ? key_at(cur + 1) : NONE;
    }
    ++steps;
  }
  if (FILL) {
    if (lane == 0)
      while (sg < nSeg) seg_end[b * nSeg + sg++] = steps;
  } else if (lane == 0) {
    w_steps[b] = steps;
  }
}

// the slot kernels' index: one row of `row` ints per step, k[W] | l[W] | a[W] | pad -- ONE LDS-DMA instruction per step
// (W = 21: 64 ints = 256 bytes with 1 int of padding; W = 64: 192 ints = 768 bytes)
__global__ void k_idx_interleave(long long n_steps, int W, int row, const int *__restrict__ st_k, const int *__restrict__ st_l,
                                 const int *__restrict__ st_a, int *__restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_steps * row) return;
  const long long st = t / row;
  const int e = (int)(t - st * row), which = e / W, sl = e - which * W;
  const int *src = which == 0 ? st_k : (which == 1 ? st_l : st_a);
  out[t] = which < 3 ? src[st * W + sl] : 0;
}

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

int mvba_set_params(mvba_handle *h, const double *X, const double *f, const double *u, const double *t, const double *R) {
  if (!h || !X || !f || !u || !t || !R) return fail(MVBA_ERR_BADARG, "null argument");
  MVBA_HIP(hipSetDevice(h->device));
  std::vector<double> cam((size_t)h->m * CAM_IN);
  for (int k = 0; k < h->m; ++k) {
    double *c = cam.data() + (size_t)k * CAM_IN;
    c[0] = f[k]; c[1] = u[2 * k]; c[2] = u[2 * k + 1];
    for (int i = 0; i < 3; ++i) c[3 + i] = t[3 * k + i];
    for (int i = 0; i < 9; ++i) c[6 + i] = R[9 * k + i];
  }
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
  for (int k = 0; k < h->m; ++k) {
    const double *c = cam.data() + (size_t)k * CAM_IN;
    f[k] = c[0]; u[2 * k] = c[1]; u[2 * k + 1] = c[2];
    for (int i = 0; i < 3; ++i) t[3 * k + i] = c[3 + i];
    for (int i = 0; i < 9; ++i) R[9 * k + i] = c[6 + i];
  }
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
void launch_resid_jac(mvba_handle *h) {  // K1 with K2 fused in, at the committed state
  const int kt = h->k1_threads;  // 8 waves share one camera table: 2 blocks = 16 waves per CU
  cam_tables(h, h->d_cam15[h->cur], nullptr);
  const int wpb = kt / 64;
  const int grid = std::max(1, std::min(2048 * 256 / kt, (h->n_tiles + wpb - 1) / wpb));
  launch_loss(h, resid_jac_kernel(h->gcam, h->loss), dim3(grid), dim3(kt), k1_lds_bytes(h->m, h->gcam, kt), h->nobs, h->m, h->d_cam15[h->cur],
              h->d_X[h->cur], h->d_obs_pt, h->d_cam, h->d_xy, h->f0, h->d_tiles, h->n_tiles, h->d_rec, h->d_PL,
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
  if (h->n_held)  // held points (mvba_set_point_hold): the masked form; without a mask the launch is the one it always was
    hipLaunchKernelGGL(k_point_inv<const uint8_t *>, dim3(std::max(grid, 1u)), dim3(256), 0, h->stream, h->N, c, h->d_PL, h->d_PB, h->d_flag,
                       h->d_Ab, nAb, h->d_prog, nprog, want_r, (const uint8_t *)h->d_held);
  else
    hipLaunchKernelGGL(k_point_inv<>, dim3(std::max(grid, 1u)), dim3(256), 0, h->stream, h->N, c, h->d_PL, h->d_PB, h->d_flag,
                       h->d_Ab, nAb, h->d_prog, nprog, want_r);
}

void launch_schur(mvba_handle *h, double c) {  // K3 in the engine's form: [A|b] of this rank's points
  const int m = h->m;
  const size_t nA = strip_offset(m, m);
  double *d_A = h->d_Ab, *d_b = h->d_Ab + nA;
  if (h->use_pairs) {
    // 64-bit offsets only when the records or the point blocks (+ the padding row) span 4 GiB (MVBA_FORCE_BIG: at test sizes too)
    const bool big = (std::max<long long>(h->nobs, h->N) + 1) * 128LL >= (1LL << 32) || h->force_big;
    if (h->schur_mode == SCHUR_SLOTS && h->slot_w == LANES_W) {
      if (h->n_waves)
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
  const size_t lds = h->gcam ? 0 : (size_t)h->m * CAM_LDS * sizeof(double);
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
  const bool sharded = h->comm || h->host_ar;
  if (local_rc && !sharded) return local_rc;
  const std::string local_err = local_rc ? g_err : std::string();
  double *d_b = h->d_Ab + strip_offset(m, m);
  if (!local_rc) {
    MVBA_HIP(hipEventRecord(ev[0], h->stream));
    // 1-4: the LM step's launches at c = 0 (K1, K3a, K3 in the engine's form, the all-reduce of [A|b])
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
                         (const double2 *)h->d_rec, (const double *)h->d_PL, (const double *)h->d_cov_sig, 1.0 / h->f0, h->d_cov_pts,
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
}  // namespace

int mvba_snapshot(mvba_handle *h) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set");
  MVBA_HIP(hipSetDevice(h->device));
  const size_t stride = snap_stride(h);
  const size_t slab = (size_t)(h->n_snap / SNAP_SLAB);
  if (slab >= h->snap_slabs.size()) {
    double *p = nullptr;
    int rc = h->mem.alloc(&p, stride * SNAP_SLAB);
    if (rc) return rc;
    h->snap_slabs.push_back(p);
  }
  double *dst = h->snap_slabs[slab] + stride * (size_t)(h->n_snap % SNAP_SLAB);
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
  const double *src = h->snap_slabs[(size_t)(i / SNAP_SLAB)] + snap_stride(h) * (size_t)(i % SNAP_SLAB);
  std::vector<double> cam((size_t)h->m * CAM_IN);
  MVBA_HIP(hipMemcpyAsync(X, src, sizeof(double) * 3 * h->N, hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipMemcpyAsync(cam.data(), src + 3 * h->N, sizeof(double) * cam.size(), hipMemcpyDeviceToHost, h->stream));
  MVBA_HIP(hipStreamSynchronize(h->stream));
  for (int k = 0; k < h->m; ++k) {
    const double *c = cam.data() + (size_t)k * CAM_IN;
    f[k] = c[0]; u[2 * k] = c[1]; u[2 * k + 1] = c[2];
    for (int q = 0; q < 3; ++q) t[3 * k + q] = c[3 + q];
    for (int q = 0; q < 9; ++q) R[9 * k + q] = c[6 + q];
  }
  return MVBA_OK;
}

int mvba_snapshot_restore(mvba_handle *h, int64_t i) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  if (i < 0 || i >= h->n_snap) return fail(MVBA_ERR_BADARG, "no such log entry");
  MVBA_HIP(hipSetDevice(h->device));
  const double *src = h->snap_slabs[(size_t)(i / SNAP_SLAB)] + snap_stride(h) * (size_t)(i % SNAP_SLAB);
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
  out8[3] = h->schur_mode | (h->schur_mode == SCHUR_SLOTS ? h->slot_w << 8 : 0);  // bits 8..15: the slot form's step width
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
