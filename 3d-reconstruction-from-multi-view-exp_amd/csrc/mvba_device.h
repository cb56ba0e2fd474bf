// What the stages of the BA device code share -- gfx950: the fixed-order sums (wave_sum, block_sum), the camera table in LDS
// or in device memory (load_cams_to_lds, stage_cams, cam_row, dxi_row),
// the gauge's kept parameters (keep_index), scalar loads of wave-uniform operands (MVBA_CONST_AS / as_const), and the constants
// of the buffers that more than one stage touches (REC, REC_C, CompactRec, LDS_CAMERAS, PBS, PACE_STRIDE, LossArgs).
//
// Included by mvba.hip first inside its device-code namespace: uses expand_cam, strip_offset, CAM_IN, CAM_LDS and DXI_LDS of mvba_common.h.
// The stage headers after it (mvba_linearize.h, mvba_schur.h, mvba_dense.h, mvba_solve.h, mvba_tail.h, mvba_cov.h, mvba_map.h)
// each use something from here.

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

constexpr int REC = 8;  // double2 slots per observation record (128 B)
// The compact record of a lane-form engine: slots 0..3 of the full one -- J_X and d/df, 64 B -- and the residual in
// an array of its own; the omega rows are (row of J_X) x (X - t) and K3 forms them again.  K1's compact instantiation takes one
// trailing argument of this type, as the robust ones take LossArgs (the full-layout instantiations none: their code is unchanged).
constexpr int REC_C = 4;
struct CompactRec {
  double2 *res;  // [n_obs + 1] residuals, the last one the padding record's zeros
};
template <typename... T>
struct is_compact_rec { static constexpr bool value = false; };
template <>
struct is_compact_rec<CompactRec> { static constexpr bool value = true; };
constexpr int LDS_CAMERAS = 646;  // cameras whose tables (K1: 18 doubles + the waves' staging tiles; K5: 28 doubles) fit one workgroup's LDS

// GCAM: beyond LDS_CAMERAS cameras the expanded camera table does not fit a workgroup's LDS next to its staging tiles; the
// kernels then read the rows of a table in device memory (k_cam_tables; 144 bytes per camera, L2-resident) through the same
// 16-byte loads.  One template parameter per kernel: the LDS form keeps its ds_read_b128, nothing is decided per access.
// cam_row / dxi_row: camera k's expanded row (its padded update row) in whichever table the kernel reads.
template <bool GCAM>
__device__ __forceinline__ const double *cam_row(const double *gcam, const double *s_cam, int k) {
  if constexpr (GCAM) return gcam + (size_t)k * CAM_LDS;
  else return s_cam + k * CAM_LDS;
}
template <bool GCAM>
__device__ __forceinline__ const double *dxi_row(const double *gdxi, const double *s_dxi, int k) {
  if constexpr (GCAM) return gdxi + (size_t)DXI_LDS * k;
  else return s_dxi + DXI_LDS * k;
}
// The LDS form's preamble: the block expands the camera table into s_cam, then the barrier (which also covers whatever else
// the kernel staged before the call).  GCAM: nothing, the table is in device memory already.
template <bool GCAM>
__device__ __forceinline__ void stage_cams(const double *cam15, int m, double f0, double *s_cam) {
  if constexpr (!GCAM) {
    load_cams_to_lds(cam15, m, f0, s_cam);
    __syncthreads();
  }
}

// Robust kernels take one trailing argument of this type (the squared instantiations none: their arguments and code are those of
// the plain kernels).  b = (delta / f0)^2, sqw = sqrt(w) per observation.
struct LossArgs {
  double b;
  double *sqw;
};

// doubles per point row of PB: one 128-byte line (k_point_inv in mvba_linearize.h writes it and has the layout)
constexpr int PBS = 16;
constexpr int PACE_STRIDE = 32;  // ints between two pacing counters: one 128-byte line each (they are hammered by ~300 waves)
