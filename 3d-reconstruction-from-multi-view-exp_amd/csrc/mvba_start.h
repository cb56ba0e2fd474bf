// What the entry points that start a reconstruction share (mvba_init.h, mvba_twoview.h, mvba_ransac.h ... mvba_match.h) -- gfx950.
//
// Included by mvba.hip after its C entry points and before mvba_init.h: uses mvba.hip's DevBufs, fail and MVBA_HIP.  Nothing
// here runs on the LM path.  
//
// One copy each of: the fixed reduction tree of a 256-thread chunk (chunk_sum; the cyclic Jacobi, its eigenvalue selection and
// INIT_REL_PIVOT are mvba_ransac_host.h's, which the host-side solves use too), the flags of a chunk counted and ranked
// (chunk_ballot, chunk_total, chunk_rank: the compactions of mvba_ransac.h and mvba_align.h), the mask step of a robust fit
// (mask_step), the host clock and the event laps (EvLaps), the checks of an observation list, of a pair list and of ascending camera
// runs, and the upload of a list.  Every floating-point sum of these entry points is taken in an order that the sizes alone
// fix: chunk_sum inside a chunk, then k_resect_combine (serial, ascending chunks) or k_twoview_combine (lane-strided, then
// the shuffle tree) over a camera's or a pair's chunks -- two orders, on purpose.

namespace {

constexpr int INIT_MAX_CAMERAS = 1704;    // (160 KiB - 256 B) / 96 B: the LDS camera table of k_project_obs
constexpr int START_CHUNK = 256;          // items (observations of a camera, points of a pair) per chunk = threads per workgroup

// The fixed tree of a chunk: the workgroup's START_CHUNK values v[e] summed into out[e] -- lanes l and l + off inside a wave,
// off = 32 .. 1, then the waves in ascending order.  Every thread of the workgroup calls it (a barrier inside).
template <int NV>
__device__ __forceinline__ void chunk_sum(const double (&v)[NV], double (&s_w)[START_CHUNK / 64][NV], double *__restrict__ out) {
  const int i = threadIdx.x;
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    double x = v[e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if ((i & 63) == 0) s_w[i >> 6][e] = x;
  }
  __syncthreads();
  if (i < NV) {
    double x = s_w[0][i];
#pragma unroll
    for (int w = 1; w < START_CHUNK / 64; ++w) x += s_w[w][i];
    out[i] = x;
  }
}

// The flags of a chunk, one per thread: the wave's ballot, with every wave's popcount in s_w.  Every thread of the workgroup
// calls it (a barrier inside); chunk_total and chunk_rank read s_w after it.
__device__ __forceinline__ unsigned long long chunk_ballot(bool flag, int (&s_w)[START_CHUNK / 64]) {
  const int i = threadIdx.x;
  const unsigned long long b = __ballot(flag);
  if ((i & 63) == 0) s_w[i >> 6] = __popcll(b);
  __syncthreads();
  return b;
}

// the number of set flags of the chunk
__device__ __forceinline__ int chunk_total(const int (&s_w)[START_CHUNK / 64]) {
  int x = 0;
#pragma unroll
  for (int w = 0; w < START_CHUNK / 64; ++w) x += s_w[w];
  return x;
}

// the number of set flags below this thread's: the lower lanes of its wave's ballot b, and the lower waves
__device__ __forceinline__ int chunk_rank(unsigned long long b, const int (&s_w)[START_CHUNK / 64]) {
  const int i = threadIdx.x;
  int j = __popcll(b & ((1ull << (i & 63)) - 1ull));
  for (int w = 0; w < (i >> 6); ++w) j += s_w[w];
  return j;
}

// The mask step of a robust fit, for one item with a model to test it against: the inlier byte, and v = (1, d2) for an inlier
// -- what chunk_sum<2> then adds up to (count, sum of d^2); v is (0, 0) beforehand, and stays so for an outlier and for a
// thread without an item.
__device__ __forceinline__ void mask_step(bool in, double d2, unsigned char *byte, double (&v)[2]) {
  *byte = in ? 1 : 0;
  if (in) { v[0] = 1.0; v[1] = d2; }
}

struct InitClock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double lap() {
    const auto t1 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
  }
};

// The event laps of one call.  create(count) makes the events; whatever was made is destroyed when the owner goes, on every
// return.  mark(stream) records the next event -- nothing without events, so a caller that times only on request creates them
// only then; again(k) records event k once more and goes on from there (marks taken once per chunk).  ms(a, b): the
// milliseconds from mark a to mark b, to be read only after a copy or a hipStreamSynchronize that follows mark b.  What a call
// reports beside its laps is the call's own rule (most of them: lap_rest of the wall time).
struct EvLaps {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  int n = 0, next = 0;
  EvLaps() = default;
  EvLaps(const EvLaps &) = delete;
  EvLaps &operator=(const EvLaps &) = delete;
  ~EvLaps() {
    for (int i = 0; i < n; ++i) hipEventDestroy(e[i]);
  }
  int create(int count) {
    for (; n < count && n < 4; ++n) MVBA_HIP(hipEventCreate(&e[n]));
    return MVBA_OK;
  }
  void mark(hipStream_t stream = 0) {
    if (next < n) hipEventRecord(e[next++], stream);
  }
  void again(int k) { next = k, mark(); }
  double ms(int a, int b) const {
    float f = 0.f;
    if (a < n && b < n) hipEventElapsedTime(&f, e[a], e[b]);
    return f;
  }
};

// the checks mvba_project makes of an observation list, with the offending number in the message
int init_check_list(int64_t n_points, int32_t n_images, const int64_t *pt_ptr, const int32_t *cam_idx, int64_t n_obs) {
  if (n_points < 0 || n_obs < 0) return fail(MVBA_ERR_BADARG, "n_points = " + std::to_string(n_points) + ", n_obs = " + std::to_string(n_obs) + ": negative size");
  if (n_images < 1) return fail(MVBA_ERR_BADARG, "n_images = " + std::to_string(n_images) + " must be at least 1");
  if (n_points >= (1LL << 31)) return fail(MVBA_ERR_BADARG, "n_points = " + std::to_string(n_points) + " must be < 2^31");
  if (!pt_ptr) {
    if (n_obs != n_points * (int64_t)n_images)
      return fail(MVBA_ERR_BADARG, "dense grid needs n_obs = n_points * n_images = " + std::to_string(n_points * (int64_t)n_images) + ", got " + std::to_string(n_obs));
    return MVBA_OK;
  }
  if (!cam_idx) return fail(MVBA_ERR_BADARG, "null argument: cam_idx (with a pt_ptr)");
  if (pt_ptr[0] != 0) return fail(MVBA_ERR_BADARG, "pt_ptr[0] = " + std::to_string(pt_ptr[0]) + " must be 0");
  for (int64_t a = 0; a < n_points; ++a)
    if (pt_ptr[a + 1] < pt_ptr[a] || pt_ptr[a + 1] > n_obs)
      return fail(MVBA_ERR_BADARG, "pt_ptr[" + std::to_string(a + 1) + "] = " + std::to_string(pt_ptr[a + 1]) + " is not ascending within n_obs = " + std::to_string(n_obs));
  if (pt_ptr[n_points] != n_obs)
    return fail(MVBA_ERR_BADARG, "pt_ptr does not span n_obs: pt_ptr[n_points] = " + std::to_string(pt_ptr[n_points]) + ", n_obs = " + std::to_string(n_obs));
  for (int64_t o = 0; o < n_obs; ++o)
    if (cam_idx[o] < 0 || cam_idx[o] >= n_images)
      return fail(MVBA_ERR_BADARG, "cam_idx out of range: cam_idx[" + std::to_string(o) + "] = " + std::to_string(cam_idx[o]) + ", n_images = " + std::to_string(n_images));
  return MVBA_OK;
}

int init_check_cameras(int32_t n_images) {
  if (n_images > INIT_MAX_CAMERAS)
    return fail(MVBA_ERR_BADARG, "too many cameras for the LDS camera table: n_images = " + std::to_string(n_images) + " (max " + std::to_string(INIT_MAX_CAMERAS) + ")");
  return MVBA_OK;
}

// a list of camera pairs (k, l): both in range, and different
int check_pairs(const int32_t *pairs, int32_t n_pairs, int32_t n_images) {
  for (int32_t p = 0; p < n_pairs; ++p) {
    const int32_t k = pairs[2 * p], l = pairs[2 * p + 1];
    if (k < 0 || k >= n_images || l < 0 || l >= n_images)
      return fail(MVBA_ERR_BADARG, "pairs[" + std::to_string(p) + "] = (" + std::to_string(k) + ", " + std::to_string(l) +
                                       "): camera index out of range, n_images = " + std::to_string(n_images));
    if (k == l) return fail(MVBA_ERR_BADARG, "pairs[" + std::to_string(p) + "] = (" + std::to_string(k) + ", " + std::to_string(l) + "): the two cameras must differ");
  }
  return MVBA_OK;
}

// the kernels that search a point's camera run (tv_find) need it to ascend; pt_ptr == nullptr: the dense grid does
int check_ascending(int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx) {
  if (!pt_ptr) return MVBA_OK;
  for (int64_t a = 0; a < n_points; ++a)
    for (int64_t o = pt_ptr[a] + 1; o < pt_ptr[a + 1]; ++o)
      if (cam_idx[o] <= cam_idx[o - 1])
        return fail(MVBA_ERR_BADARG, "cam_idx is not ascending within point " + std::to_string(a) + ": cam_idx[" + std::to_string(o) + "] = " +
                                         std::to_string(cam_idx[o]) + " after " + std::to_string(cam_idx[o - 1]));
  return MVBA_OK;
}

// An observation list to the device, owned by tmp: xy (unless nullptr) into *dxy, and pt_ptr and cam_idx into *dptr and
// *dcam, which stay nullptr for the dense grid (pt_ptr == nullptr).
int upload_list(DevBufs &tmp, int64_t n_points, int64_t n_obs, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy,
                long long **dptr, int **dcam, double2 **dxy) {
  static_assert(sizeof(long long) == sizeof(int64_t), "pt_ptr goes to the device as it is");
  int rc;
  if (xy) {
    if ((rc = tmp.alloc(dxy, (size_t)n_obs))) return rc;
    if (n_obs) MVBA_HIP(hipMemcpy(*dxy, xy, sizeof(double2) * n_obs, hipMemcpyHostToDevice));
  }
  if (pt_ptr) {
    if ((rc = tmp.alloc(dptr, (size_t)n_points + 1)) || (rc = tmp.alloc(dcam, (size_t)n_obs))) return rc;
    MVBA_HIP(hipMemcpy(*dptr, pt_ptr, sizeof(int64_t) * (n_points + 1), hipMemcpyHostToDevice));
    if (n_obs) MVBA_HIP(hipMemcpy(*dcam, cam_idx, sizeof(int) * n_obs, hipMemcpyHostToDevice));
  }
  return MVBA_OK;
}

}  // namespace
