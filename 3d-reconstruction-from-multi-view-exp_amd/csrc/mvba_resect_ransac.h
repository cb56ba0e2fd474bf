// Robust resection (mvba_resect_robust, mvba_resect_sample): 6-point RANSAC for camera matrices -- kernels and host code,
// gfx950.
//
// Included by mvba.hip after mvba_ransac.h: uses its rs_sample, RS_HYP_BLOCK, RS_MAX_HYP, RS_MAX_REFIT and state bits,
// mvba_twoview.h's tv_pair_tile, mvba_init.h's resect_build_list, rs_pass, k_resect_chunk, k_resect_combine, k_resect_norm,
// resect_solve_camera and resect_denormalise, mvba_start.h's chunk_sum, init_check_list, InitClock and INIT_REL_PIVOT, and
// mvba.hip's DevBufs, fail and MVBA_HIP.  Nothing here runs on the LM path.  
//
// The usable observations are sorted camera-major on the host as for mvba_resect, so a camera's observations are a dense run
// in ascending point order: sample index j of camera k is entry cam_ptr[k] + j.  The listed cameras (duplicates allowed) get
// their own chunk list of 256-observation chunks; every per-camera array is indexed by the position in the list.  One THREAD
// per hypothesis draws its 6 indices, sums the 40 moments in registers (static indices), builds the 12 x 12 matrix the way
// resect_solve_camera does and diagonalises it by cyclic Jacobi with A and V in LDS, element-major (element e of thread t at
// [e x 64 + t], as k_ransac_hyp does at order 9).  The scoring kernel holds 64 camera matrices in LDS, one observation per
// thread; a hypothesis's count is ballot + popcount per wave, then integer atomics (LDS, then device memory): exact in any
// order.  Refits sum the passes of k_resect_chunk under a byte mask; the order-12 eigen-problem and the denormalisation are
// resect_solve_camera's, on the host.  No floating-point atomics.

namespace {

constexpr int RR_MIN_OBS = 6;          // the linear solution needs 12 rows
constexpr size_t RR_HYP_BYTES = 100;   // device bytes per hypothesis of a camera of a tile: 96 P, 4 count

// depth and squared reprojection distance of one observation under P; inlier: in front and within thr2
__device__ __forceinline__ bool rr_inlier(const double *P, const double *Xa, double2 z, double thr2, double &d2) {
  const double p0 = Xa[0] * P[0] + Xa[1] * P[1] + Xa[2] * P[2] + P[3];
  const double p1 = Xa[0] * P[4] + Xa[1] * P[5] + Xa[2] * P[6] + P[7];
  const double p2 = Xa[0] * P[8] + Xa[1] * P[9] + Xa[2] * P[10] + P[11];
  const double r0 = p0 / p2 - z.x, r1 = p1 / p2 - z.y;
  d2 = r0 * r0 + r1 * r1;
  return p2 > 0.0 && d2 <= thr2;
}

// k_resect_chunk's passes 0, 1, 2 over the observations whose byte in the camera's current mask is set.  The chunks are
// those of the listed cameras (ch_cam: the position in the list; ch_mask: the chunk's offset in the mask buffers); a camera
// that is not RS_ACTIVE sums nothing.
template <int MODE>
__global__ __launch_bounds__(START_CHUNK) void k_resect_fit(const int *__restrict__ ch_cam, const long long *__restrict__ ch_start,
                                                            const long long *__restrict__ ch_mask, const int *__restrict__ ch_cnt,
                                                            const int *__restrict__ cm_pt, const double2 *__restrict__ cm_xy,
                                                            const double *__restrict__ X, const int *__restrict__ state,
                                                            const unsigned char *__restrict__ inl0, const unsigned char *__restrict__ inl1,
                                                            const double *__restrict__ aux, double *__restrict__ part) {
  constexpr int NV = rs_values(MODE);
  __shared__ double s_w[START_CHUNK / 64][NV];
  const int c = blockIdx.x, k = ch_cam[c], i = threadIdx.x, st = state[k];
  double v[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = 0.0;
  if ((st & RS_ACTIVE) && i < ch_cnt[c] && ((st & RS_CUR) ? inl1 : inl0)[ch_mask[c] + i]) {
    const long long o = ch_start[c] + i;
    rs_pass<MODE>(X + 3 * (size_t)cm_pt[o], cm_xy[o], MODE == 0 ? aux : aux + RS_NORM * (size_t)k, v);
  }
  chunk_sum<NV>(v, s_w, part + (size_t)c * NV);
}

// One thread per hypothesis of camera cam0 + blockIdx.y of the list: sample, the 40 sums over the 6 normalised observations,
// the 12 x 12 moment matrix, cyclic Jacobi in LDS, p^ = the eigenvector of the smallest eigenvalue, P = p^ denormalised and
// scaled -> hypP [tile camera][H][12]; hyp_count = 0, or -1 (and a NaN matrix) if degenerate.
__global__ __launch_bounds__(RS_HYP_BLOCK) void k_resect_hyp(int cam0, int H, unsigned long long seed, const int *__restrict__ cams,
                                                             const long long *__restrict__ lc_start, const int *__restrict__ lc_n,
                                                             const int *__restrict__ cm_pt, const double2 *__restrict__ cm_xy,
                                                             const double *__restrict__ X, const double *__restrict__ norm,
                                                             double *__restrict__ hypP, int *__restrict__ hyp_count) {
  extern __shared__ double s_rr[];  // A [144][64], V [144][64]
  const int kl = blockIdx.y, k = cam0 + kl, tid = threadIdx.x, h = blockIdx.x * RS_HYP_BLOCK + tid;
  if (h >= H) return;  // (no barrier below: a thread works on its own LDS column)
  const size_t oh = (size_t)kl * H + h;
  const int n = lc_n[k];
  bool good = n >= RR_MIN_OBS;  // (below 6 the rejection loop of rs_sample would not end)
  double P[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) P[e] = NAN;
  if (good) {
    double *sA = s_rr + tid, *sV = s_rr + 144 * RS_HYP_BLOCK + tid;
    auto A = [&](int r, int c) -> double & { return sA[(r * 12 + c) * RS_HYP_BLOCK]; };
    auto V = [&](int r, int c) -> double & { return sV[(r * 12 + c) * RS_HYP_BLOCK]; };
    const double *nm = norm + RS_NORM * (size_t)k;
    long long idx[6];
    rs_sample(seed, cams[k], cams[k], h, n, idx);
    double S[40];
#pragma unroll
    for (int e = 0; e < 40; ++e) S[e] = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const long long o = lc_start[k] + idx[c];
      double v[40];
      rs_pass<2>(X + 3 * (size_t)cm_pt[o], cm_xy[o], nm, v);
#pragma unroll
      for (int e = 0; e < 40; ++e) S[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < 40; ++e) good = good && isfinite(S[e]);
    for (int e = 0; e < 144; ++e) {
      sA[e * RS_HYP_BLOCK] = 0.0;
      sV[e * RS_HYP_BLOCK] = (e % 13 == 0) ? 1.0 : 0.0;
    }
    {  // resect_solve_camera's matrix from the 40 sums
      int e = 0;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b, ++e) {
          const double hh = S[e], xh = S[10 + e], yh = S[20 + e], wh = S[30 + e];
          A(a, b) = hh; A(b, a) = hh;
          A(4 + a, 4 + b) = hh; A(4 + b, 4 + a) = hh;
          A(a, 8 + b) = -xh; A(b, 8 + a) = -xh; A(8 + b, a) = -xh; A(8 + a, b) = -xh;
          A(4 + a, 8 + b) = -yh; A(4 + b, 8 + a) = -yh; A(8 + b, 4 + a) = -yh; A(8 + a, 4 + b) = -yh;
          A(8 + a, 8 + b) = wh; A(8 + b, 8 + a) = wh;
        }
    }
    // sym_eig_jacobi's rotations and stopping rule, with run-time indices into LDS
    for (int sweep = 0; sweep < 30 && good; ++sweep) {
      bool any = false;
      for (int a = 0; a < 11; ++a)
        for (int b = a + 1; b < 12; ++b) {
          const double apq = A(a, b), app = A(a, a), aqq = A(b, b);
          const double g = fabs(apq);
          if (!(g > 0.0) || (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq))) {
            A(a, b) = A(b, a) = 0.0;
            continue;
          }
          any = true;
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
          A(a, a) = app - t * apq;
          A(b, b) = aqq + t * apq;
          A(a, b) = A(b, a) = 0.0;
          for (int r = 0; r < 12; ++r) {
            if (r != a && r != b) {
              const double arp = A(r, a), arq = A(r, b);
              A(r, a) = A(a, r) = arp - s * (arq + tau * arp);
              A(r, b) = A(b, r) = arq + s * (arp - tau * arq);
            }
            const double vrp = V(r, a), vrq = V(r, b);
            V(r, a) = vrp - s * (vrq + tau * vrp);
            V(r, b) = vrq + s * (vrp - tau * vrq);
          }
        }
      if (!any) break;
    }
    if (good) {
      int best = 0;
      double l1 = A(0, 0), lmax = A(0, 0), l2 = HUGE_VAL;
      for (int e = 1; e < 12; ++e) {
        const double d = A(e, e);
        if (d < l1) { l1 = d; best = e; }
        lmax = fmax(lmax, d);
      }
      for (int e = 0; e < 12; ++e)
        if (e != best) l2 = fmin(l2, A(e, e));
      good = l2 > INIT_REL_PIVOT * lmax;
      double p[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) p[e] = V(e, best);
      good = resect_denormalise(p, nm, P) && good;
    }
  }
#pragma unroll
  for (int e = 0; e < 12; ++e) hypP[oh * 12 + e] = good ? P[e] : NAN;
  hyp_count[oh] = good ? 0 : -1;
}

// Scoring: grid (the chunks of the tile's cameras, blocks of 64 hypotheses).  A thread holds one observation and walks the
// block's matrices in LDS (every lane reads the same address: a broadcast); a hypothesis's inliers of a wave are one ballot
// and one popcount, kept by the lane of the hypothesis's number; then integer atomics.  A degenerate hypothesis is NaN: no
// observation passes, its count stays -1.
__global__ __launch_bounds__(START_CHUNK) void k_resect_score(int cam0, int H, const int *__restrict__ ch_cam, const long long *__restrict__ ch_start,
                                                              const int *__restrict__ ch_cnt, const int *__restrict__ lc_n,
                                                              const int *__restrict__ cm_pt, const double2 *__restrict__ cm_xy,
                                                              const double *__restrict__ X, const double *__restrict__ hypP, double thr2,
                                                              int *__restrict__ hyp_count) {
  __shared__ double s_P[RS_HYP_BLOCK * 12];
  __shared__ int s_cnt[RS_HYP_BLOCK];
  const int c = blockIdx.x, k = ch_cam[c], kl = k - cam0, h0 = blockIdx.y * RS_HYP_BLOCK, i = threadIdx.x, lane = i & 63;
  if (lc_n[k] < RR_MIN_OBS) return;  // (the whole workgroup leaves: every count of the camera is -1)
  const int nh = min(RS_HYP_BLOCK, H - h0);
  for (int e = i; e < nh * 12; e += START_CHUNK) s_P[e] = hypP[((size_t)kl * H + h0) * 12 + e];
  if (i < RS_HYP_BLOCK) s_cnt[i] = 0;
  __syncthreads();
  const bool live = i < ch_cnt[c];
  double Xa[3] = {0.0, 0.0, 0.0};
  double2 z = make_double2(0.0, 0.0);
  if (live) {
    const long long o = ch_start[c] + i;
    const double *Xp = X + 3 * (size_t)cm_pt[o];
    Xa[0] = Xp[0]; Xa[1] = Xp[1]; Xa[2] = Xp[2];
    z = cm_xy[o];
  }
  int mine = 0;
  for (int hh = 0; hh < nh; ++hh) {
    double d2;
    const bool in = rr_inlier(s_P + 12 * hh, Xa, z, thr2, d2);
    const int cnt = __popcll(__ballot(live && in));
    if (lane == hh) mine = cnt;
  }
  if (mine) atomicAdd(&s_cnt[lane], mine);
  __syncthreads();
  if (i < nh && s_cnt[i]) atomicAdd(&hyp_count[(size_t)kl * H + h0 + i], s_cnt[i]);
}

// Pcur[camera] = the matrix of the camera's best hypothesis (best < 0: NaN), for the cnt cameras of a tile
__global__ __launch_bounds__(256) void k_resect_gather(int cnt, int H, const int *__restrict__ best, const double *__restrict__ hypP,
                                                       double *__restrict__ Pcur) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cnt * 12) return;
  const int kl = t / 12, e = t - 12 * kl, b = best[kl];
  Pcur[t] = b >= 0 ? hypP[((size_t)kl * H + b) * 12 + e] : NAN;
}

// The inlier set of P[camera] into the camera's OTHER mask buffer, and part[chunk][2] = (count, sum of d^2 over it) by the
// tree of chunk_sum (the count is exact in a double).  A camera that is not RS_ACTIVE writes nothing and sums nothing.
__global__ __launch_bounds__(START_CHUNK) void k_resect_mask(const int *__restrict__ ch_cam, const long long *__restrict__ ch_start,
                                                             const long long *__restrict__ ch_mask, const int *__restrict__ ch_cnt,
                                                             const int *__restrict__ cm_pt, const double2 *__restrict__ cm_xy,
                                                             const double *__restrict__ X, const int *__restrict__ state,
                                                             const double *__restrict__ P, double thr2, unsigned char *__restrict__ inl0,
                                                             unsigned char *__restrict__ inl1, double *__restrict__ part) {
  __shared__ double s_w[START_CHUNK / 64][2];
  const int c = blockIdx.x, k = ch_cam[c], i = threadIdx.x, st = state[k];
  double v[2] = {0.0, 0.0};
  if ((st & RS_ACTIVE) && i < ch_cnt[c]) {
    const long long o = ch_start[c] + i;
    double d2;
    const bool in = rr_inlier(P + 12 * (size_t)k, X + 3 * (size_t)cm_pt[o], cm_xy[o], thr2, d2);
    ((st & RS_CUR) ? inl0 : inl1)[ch_mask[c] + i] = in ? 1 : 0;
    if (in) { v[0] = 1.0; v[1] = d2; }
  }
  chunk_sum<2>(v, s_w, part + (size_t)c * 2);
}

// out[the observation's index in the caller's list] = 1 for the observations of the camera's current mask (cameras of status
// 0; out is zero beforehand)
__global__ __launch_bounds__(START_CHUNK) void k_resect_scatter(const int *__restrict__ ch_cam, const long long *__restrict__ ch_start,
                                                                const long long *__restrict__ ch_mask, const int *__restrict__ ch_cnt,
                                                                const long long *__restrict__ cm_obs, const int *__restrict__ state,
                                                                const unsigned char *__restrict__ inl0, const unsigned char *__restrict__ inl1,
                                                                unsigned char *__restrict__ out) {
  const int c = blockIdx.x, i = threadIdx.x, st = state[ch_cam[c]];
  if (!(st & RS_OK) || i >= ch_cnt[c]) return;
  if (((st & RS_CUR) ? inl1 : inl0)[ch_mask[c] + i]) out[cm_obs[ch_start[c] + i]] = 1;
}

}  // namespace

extern "C" {

int mvba_resect_sample(uint64_t seed, int32_t k, int32_t h, int64_t n, int64_t *idx6) {
  if (!idx6) return fail(MVBA_ERR_BADARG, "null argument: idx6 (argument 5)");
  if (n < RR_MIN_OBS || n >= (1LL << 31)) return fail(MVBA_ERR_BADARG, "n = " + std::to_string(n) + " must be in 6 .. 2^31 - 1");
  if (k < 0 || h < 0) return fail(MVBA_ERR_BADARG, "k = " + std::to_string(k) + ", h = " + std::to_string(h) + ": negative index");
  long long idx[6];
  rs_sample(seed, k, k, h, n, idx);
  for (int c = 0; c < 6; ++c) idx6[c] = idx[c];
  return MVBA_OK;
}

int mvba_resect_robust(const double *X, int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int64_t n_obs,
                       int32_t n_images, const uint8_t *point_ok, const int32_t *cameras, int32_t n_cameras, double threshold,
                       int32_t n_hypotheses, uint64_t seed, int32_t n_refit, double *P, double *quality, int64_t *n_usable,
                       int64_t *n_inliers, int32_t *best, uint8_t *inlier, int32_t *hyp_count, int32_t *status, double *timings_ms,
                       int32_t device) {
  if (n_cameras < 0) return fail(MVBA_ERR_BADARG, "n_cameras = " + std::to_string(n_cameras) + " must be >= 0");
  if (!X || !xy || (n_cameras > 0 && !P))
    return fail(MVBA_ERR_BADARG, std::string("null argument: ") + (!X ? "X" : (!xy ? "xy" : "P")) + " (argument " + std::to_string(!X ? 1 : (!xy ? 5 : 15)) + ")");
  if (!std::isfinite(threshold) || !(threshold > 0.0))
    return fail(MVBA_ERR_BADARG, "threshold = " + std::to_string(threshold) + " must be finite and > 0");
  if (n_hypotheses < 1 || n_hypotheses > RS_MAX_HYP)
    return fail(MVBA_ERR_BADARG, "n_hypotheses = " + std::to_string(n_hypotheses) + " must be in 1 .. " + std::to_string(RS_MAX_HYP));
  if (n_refit < 0 || n_refit > RS_MAX_REFIT)
    return fail(MVBA_ERR_BADARG, "n_refit = " + std::to_string(n_refit) + " must be in 0 .. " + std::to_string(RS_MAX_REFIT));
  int rc = init_check_list(n_points, n_images, pt_ptr, cam_idx, n_obs);
  if (rc) return rc;
  const int m = n_images;
  if (!cameras && n_cameras != m)
    return fail(MVBA_ERR_BADARG, "cameras = NULL lists every camera: n_cameras = " + std::to_string(n_cameras) + " must be n_images = " + std::to_string(m));
  for (int32_t c = 0; cameras && c < n_cameras; ++c)
    if (cameras[c] < 0 || cameras[c] >= m)
      return fail(MVBA_ERR_BADARG, "cameras[" + std::to_string(c) + "] = " + std::to_string(cameras[c]) + ": camera index out of range, n_images = " + std::to_string(m));
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = timings_ms[3] = 0.0;
  const int nl = n_cameras, H = n_hypotheses;
  const double thr2 = threshold * threshold;
  // the defaults are those of a camera without usable observations: status 1
  for (int c = 0; c < nl; ++c) {
    for (int j = 0; j < 12; ++j) P[12 * (size_t)c + j] = NAN;
    if (quality) quality[2 * c] = quality[2 * c + 1] = NAN;
    if (n_usable) n_usable[c] = 0;
    if (n_inliers) n_inliers[c] = 0;
    if (best) best[c] = -1;
    if (status) status[c] = 1;
  }
  if (inlier && n_obs) std::memset(inlier, 0, (size_t)n_obs);
  if (hyp_count) std::fill(hyp_count, hyp_count + (size_t)nl * H, -1);
  if (nl == 0) return MVBA_OK;

  InitClock clk;
  ResectList list;
  resect_build_list(X, n_points, pt_ptr, cam_idx, xy, m, point_ok, inlier != nullptr, list);
  const long long n_used = list.cam_ptr[m];
  // the listed cameras' runs and chunks; a listed camera's bytes in the mask buffers start at its lc_mask
  std::vector<int> cams((size_t)nl), lc_n((size_t)nl), lc_ch((size_t)nl + 1, 0), ch_cam, ch_cnt;
  std::vector<long long> lc_start((size_t)nl), ch_start, ch_mask;
  long long n_mask = 0;
  for (int c = 0; c < nl; ++c) {
    const int k = cameras ? cameras[c] : c;
    const long long n = list.cam_ptr[k + 1] - list.cam_ptr[k];
    if (n >= (1LL << 31)) return fail(MVBA_ERR_BADARG, "camera " + std::to_string(k) + " has " + std::to_string(n) + " usable observations: must be < 2^31");
    cams[c] = k;
    lc_n[c] = (int)n;
    lc_start[c] = list.cam_ptr[k];
    if (n_usable) n_usable[c] = n;
    for (long long s = 0; s < n; s += START_CHUNK) {
      ch_cam.push_back(c);
      ch_start.push_back(list.cam_ptr[k] + s);
      ch_mask.push_back(n_mask + s);
      ch_cnt.push_back((int)std::min<long long>(START_CHUNK, n - s));
    }
    n_mask += n;
    if (ch_cam.size() > (size_t)0x7fffffff) return fail(MVBA_ERR_BADARG, "too many chunks of 256 observations over the listed cameras");
    lc_ch[c + 1] = (int)ch_cam.size();
  }
  const int n_ch = (int)ch_cam.size();
  if (n_ch == 0) {
    if (timings_ms) timings_ms[0] = clk.lap();
    return MVBA_OK;
  }

  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  const int tile = tv_pair_tile(nl, RR_HYP_BYTES * (size_t)H);
  DevBufs tmp;
  double *dX = nullptr, *dpart = nullptr, *dS = nullptr, *dnorm = nullptr, *dnorm2 = nullptr, *dP = nullptr, *dhypP = nullptr;
  double2 *dxy = nullptr;
  int *dpt = nullptr, *dcams = nullptr, *dlc_n = nullptr, *dlc_ch = nullptr, *dch_cam = nullptr, *dch_cnt = nullptr, *dstate = nullptr,
      *dbest = nullptr, *dhc = nullptr;
  long long *dlc_start = nullptr, *dch_start = nullptr, *dch_mask = nullptr, *dobs = nullptr;
  unsigned char *dinl0 = nullptr, *dinl1 = nullptr, *dout = nullptr;
  if ((rc = tmp.alloc(&dX, 3 * (size_t)n_points)) || (rc = tmp.alloc(&dxy, (size_t)n_used)) || (rc = tmp.alloc(&dpt, (size_t)n_used)) ||
      (rc = tmp.alloc(&dcams, (size_t)nl)) || (rc = tmp.alloc(&dlc_n, (size_t)nl)) || (rc = tmp.alloc(&dlc_start, (size_t)nl)) ||
      (rc = tmp.alloc(&dlc_ch, (size_t)nl + 1)) || (rc = tmp.alloc(&dch_cam, (size_t)n_ch)) || (rc = tmp.alloc(&dch_cnt, (size_t)n_ch)) ||
      (rc = tmp.alloc(&dch_start, (size_t)n_ch)) || (rc = tmp.alloc(&dch_mask, (size_t)n_ch)) || (rc = tmp.alloc(&dpart, 40 * (size_t)n_ch)) ||
      (rc = tmp.alloc(&dS, 40 * (size_t)tile)) || (rc = tmp.alloc(&dnorm, RS_NORM * (size_t)nl)) || (rc = tmp.alloc(&dnorm2, RS_NORM * (size_t)nl)) ||
      (rc = tmp.alloc(&dP, 12 * (size_t)nl)) || (rc = tmp.alloc(&dstate, (size_t)nl)) || (rc = tmp.alloc(&dbest, (size_t)tile)) ||
      (rc = tmp.alloc(&dhc, (size_t)tile * H)) || (rc = tmp.alloc(&dhypP, 12 * (size_t)tile * H)) || (rc = tmp.alloc(&dinl0, (size_t)n_mask)) ||
      (rc = tmp.alloc(&dinl1, (size_t)n_mask)))
    return rc;
  if (inlier && ((rc = tmp.alloc(&dout, (size_t)n_obs)) || (rc = tmp.alloc(&dobs, (size_t)n_used)))) return rc;
  MVBA_HIP(hipMemcpy(dX, X, sizeof(double) * 3 * n_points, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dxy, list.cm_xy.data(), sizeof(double2) * n_used, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dpt, list.cm_pt.data(), sizeof(int) * n_used, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dcams, cams.data(), sizeof(int) * nl, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dlc_n, lc_n.data(), sizeof(int) * nl, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dlc_start, lc_start.data(), sizeof(long long) * nl, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dlc_ch, lc_ch.data(), sizeof(int) * (nl + 1), hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dch_cam, ch_cam.data(), sizeof(int) * n_ch, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dch_cnt, ch_cnt.data(), sizeof(int) * n_ch, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dch_start, ch_start.data(), sizeof(long long) * n_ch, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(dch_mask, ch_mask.data(), sizeof(long long) * n_ch, hipMemcpyHostToDevice));
  if (inlier) {
    MVBA_HIP(hipMemcpy(dobs, list.cm_obs.data(), sizeof(long long) * n_used, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemset(dout, 0, (size_t)n_obs));
  }
  const int hyp_lds = (int)(sizeof(double) * 2 * 144 * RS_HYP_BLOCK);
  MVBA_HIP(hipFuncSetAttribute((const void *)k_resect_hyp, hipFuncAttributeMaxDynamicSharedMemorySize, hyp_lds));
  double t_up = clk.lap(), t_score = 0.0, t_refit = 0.0, t_rest = 0.0;

  const dim3 b256(256), bch(START_CHUNK);
  const int hb = (H + RS_HYP_BLOCK - 1) / RS_HYP_BLOCK;
  std::vector<int> hc((size_t)tile * H), bst((size_t)tile), state((size_t)nl, 0), st((size_t)tile);
  std::vector<long long> nin((size_t)tile);
  std::vector<double> S(40 * (size_t)tile), norm(RS_NORM * (size_t)tile), Pc(12 * (size_t)tile), Pn(12 * (size_t)tile), S2(2 * (size_t)tile),
      ssq((size_t)tile), ratio((size_t)tile), rt((size_t)tile);
  for (int c0 = 0; c0 < nl; c0 += tile) {
    const int cnt = std::min(tile, nl - c0), ch0 = lc_ch[c0], tch = lc_ch[c0 + cnt] - ch0;
    const dim3 gch((unsigned)std::max(tch, 1)), gc((cnt + 255) / 256);
    const int *tcam = dch_cam + ch0, *tcnt = dch_cnt + ch0;
    const long long *tstart = dch_start + ch0, *tmask = dch_mask + ch0;
    int *tstate = state.data() + c0;
    // (a tile's sums: dS [cnt][nv], of the chunk partials at their global place in dpart)
    auto combine = [&](int nv) { hipLaunchKernelGGL(k_resect_combine, dim3((cnt * nv + 255) / 256), b256, 0, 0, cnt, nv, dlc_ch + c0, dpart, dS); };
    auto put_state = [&]() -> int {
      MVBA_HIP(hipMemcpy(dstate + c0, tstate, sizeof(int) * cnt, hipMemcpyHostToDevice));
      return MVBA_OK;
    };
    // the inlier sets of dP under the cameras' states: counts and sums of d^2 into S2
    auto mask = [&]() -> int {
      int r = put_state();
      if (r) return r;
      if (tch > 0) hipLaunchKernelGGL(k_resect_mask, gch, bch, 0, 0, tcam, tstart, tmask, tcnt, dpt, dxy, dX, dstate, dP, thr2, dinl0, dinl1, dpart + 2 * (size_t)ch0);
      combine(2);
      MVBA_HIP(hipGetLastError());
      MVBA_HIP(hipMemcpy(S2.data(), dS, sizeof(double) * 2 * cnt, hipMemcpyDeviceToHost));
      return MVBA_OK;
    };

    // normalisation over all usable observations (mvba_resect's passes 0 and 1), hypotheses, scores
    if (tch > 0) {
      hipLaunchKernelGGL(k_resect_chunk<0>, gch, bch, 0, 0, tcam, tstart, tcnt, dpt, dxy, dX, (const double *)nullptr, dpart + 6 * (size_t)ch0);
      combine(6);
      hipLaunchKernelGGL(k_resect_norm, gc, b256, 0, 0, cnt, 0, dS, dnorm + RS_NORM * (size_t)c0);
      hipLaunchKernelGGL(k_resect_chunk<1>, gch, bch, 0, 0, tcam, tstart, tcnt, dpt, dxy, dX, dnorm, dpart + 2 * (size_t)ch0);
      combine(2);
      hipLaunchKernelGGL(k_resect_norm, gc, b256, 0, 0, cnt, 1, dS, dnorm + RS_NORM * (size_t)c0);
    }
    hipLaunchKernelGGL(k_resect_hyp, dim3(hb, cnt), dim3(RS_HYP_BLOCK), hyp_lds, 0, c0, H, (unsigned long long)seed, dcams, dlc_start, dlc_n, dpt, dxy,
                       dX, dnorm, dhypP, dhc);
    if (tch > 0)
      hipLaunchKernelGGL(k_resect_score, dim3((unsigned)tch, hb), bch, 0, 0, c0, H, tcam, tstart, tcnt, dlc_n, dpt, dxy, dX, dhypP, thr2, dhc);
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(hc.data(), dhc, sizeof(int) * (size_t)cnt * H, hipMemcpyDeviceToHost));
    t_score += clk.lap();

    // arg-max on the host: the largest count, the lowest h on ties
    for (int p = 0; p < cnt; ++p) {
      const int *c = hc.data() + (size_t)p * H;
      int b = 0;
      for (int h = 1; h < H; ++h)
        if (c[h] > c[b]) b = h;
      st[p] = lc_n[c0 + p] < RR_MIN_OBS ? 1 : (c[b] < 0 ? 2 : (c[b] < RR_MIN_OBS ? 4 : 0));
      bst[p] = c[b] < 0 ? -1 : b;  // (status 1 and 2: every count is -1)
      tstate[p] = st[p] == 0 ? (RS_OK | RS_ACTIVE | RS_CUR) : 0;  // (the first mask goes into buffer 0)
    }
    MVBA_HIP(hipMemcpy(dbest, bst.data(), sizeof(int) * cnt, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_resect_gather, dim3((cnt * 12 + 255) / 256), b256, 0, 0, cnt, H, dbest, dhypP, dP + 12 * (size_t)c0);
    if ((rc = mask())) return rc;
    MVBA_HIP(hipMemcpy(Pc.data(), dP + 12 * (size_t)c0, sizeof(double) * 12 * cnt, hipMemcpyDeviceToHost));
    int n_active = 0;
    for (int p = 0; p < cnt; ++p) {
      if (st[p]) continue;
      tstate[p] ^= RS_CUR;
      nin[p] = (long long)S2[2 * p];
      ssq[p] = S2[2 * p + 1];
      ratio[p] = 0.0;  // (no refit kept yet)
      ++n_active;
    }
    t_rest += clk.lap();

    // refits: mvba_resect's fit on the current inliers alone.  The first is kept if it has 6 inliers of its own (the minimal
    // 6-point matrix is too ill-conditioned to hold the full fit to its count), a later one while its set does not shrink
    for (int r = 0; r < n_refit && n_active > 0; ++r) {
      if ((rc = put_state())) return rc;
      double *tn = dnorm2 + RS_NORM * (size_t)c0;
      hipLaunchKernelGGL(k_resect_fit<0>, gch, bch, 0, 0, tcam, tstart, tmask, tcnt, dpt, dxy, dX, dstate, dinl0, dinl1, (const double *)nullptr, dpart + 6 * (size_t)ch0);
      combine(6);
      hipLaunchKernelGGL(k_resect_norm, gc, b256, 0, 0, cnt, 0, dS, tn);
      hipLaunchKernelGGL(k_resect_fit<1>, gch, bch, 0, 0, tcam, tstart, tmask, tcnt, dpt, dxy, dX, dstate, dinl0, dinl1, dnorm2, dpart + 2 * (size_t)ch0);
      combine(2);
      hipLaunchKernelGGL(k_resect_norm, gc, b256, 0, 0, cnt, 1, dS, tn);
      hipLaunchKernelGGL(k_resect_fit<2>, gch, bch, 0, 0, tcam, tstart, tmask, tcnt, dpt, dxy, dX, dstate, dinl0, dinl1, dnorm2, dpart + 40 * (size_t)ch0);
      combine(40);
      MVBA_HIP(hipGetLastError());
      MVBA_HIP(hipMemcpy(S.data(), dS, sizeof(double) * 40 * cnt, hipMemcpyDeviceToHost));
      MVBA_HIP(hipMemcpy(norm.data(), tn, sizeof(double) * RS_NORM * cnt, hipMemcpyDeviceToHost));
      std::fill(rt.begin(), rt.end(), NAN);
      for (int p = 0; p < cnt; ++p) {
        for (int j = 0; j < 12; ++j) Pn[12 * (size_t)p + j] = NAN;
        if (!(tstate[p] & RS_ACTIVE)) continue;
        if (resect_solve_camera(S.data() + 40 * (size_t)p, norm.data() + RS_NORM * (size_t)p, Pn.data() + 12 * (size_t)p, &rt[p])) {
          tstate[p] &= ~RS_ACTIVE;
          --n_active;
        }
      }
      if (n_active == 0) break;
      MVBA_HIP(hipMemcpy(dP + 12 * (size_t)c0, Pn.data(), sizeof(double) * 12 * cnt, hipMemcpyHostToDevice));
      if ((rc = mask())) return rc;
      for (int p = 0; p < cnt; ++p) {
        if (!(tstate[p] & RS_ACTIVE)) continue;
        const long long c = (long long)S2[2 * p];
        if (c >= (r == 0 ? (long long)RR_MIN_OBS : nin[p])) {
          tstate[p] ^= RS_CUR;
          nin[p] = c;
          ssq[p] = S2[2 * p + 1];
          ratio[p] = rt[p];
          for (int j = 0; j < 12; ++j) Pc[12 * (size_t)p + j] = Pn[12 * (size_t)p + j];
        } else {
          tstate[p] &= ~RS_ACTIVE;
          --n_active;
        }
      }
    }
    t_refit += clk.lap();

    if (inlier && tch > 0) {
      if ((rc = put_state())) return rc;
      hipLaunchKernelGGL(k_resect_scatter, gch, bch, 0, 0, tcam, tstart, tmask, tcnt, dobs, dstate, dinl0, dinl1, dout);
      MVBA_HIP(hipGetLastError());
    }
    for (int p = 0; p < cnt; ++p) {
      const size_t g = (size_t)c0 + p;
      if (status) status[g] = st[p];
      if (best) best[g] = bst[p];
      if (hyp_count) std::copy(hc.begin() + (size_t)p * H, hc.begin() + (size_t)(p + 1) * H, hyp_count + g * H);
      if (st[p]) continue;
      for (int j = 0; j < 12; ++j) P[12 * g + j] = Pc[12 * (size_t)p + j];
      if (n_inliers) n_inliers[g] = nin[p];
      if (quality) {
        quality[2 * g] = sqrt(ssq[p] / (double)nin[p]);
        quality[2 * g + 1] = ratio[p];
      }
    }
    t_rest += clk.lap();
  }
  if (inlier) MVBA_HIP(hipMemcpy(inlier, dout, (size_t)n_obs, hipMemcpyDeviceToHost));
  t_rest += clk.lap();
  if (timings_ms) {
    timings_ms[0] = t_up;
    timings_ms[1] = t_score;
    timings_ms[2] = t_refit;
    timings_ms[3] = t_rest;
  }
  return MVBA_OK;
}

}  // extern "C"
