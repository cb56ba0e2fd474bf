// Robust resection (mvba_resect_robust, mvba_resect_sample): 6-point RANSAC for camera matrices -- kernels and host code,
// gfx950.
//
// Included by mvba.hip after mvba_ransac.h: uses its rs_sample, sample_entry, rs_lds_eig, rs_score_block, rs_score_add and
// RS_HYP_BLOCK, mvba_ransac_host.h's argument checks, RsTile, rs_stop, rs_current, rs_other, RsLaps and state bits,
// mvba_twoview.h's tv_pair_tile, mvba_init.h's resect_build_list, CamWork, rs_pass, k_resect_chunk, k_resect_combine,
// k_resect_norm, resect_solve_camera and resect_denormalise, mvba_start.h's chunk_sum, mask_step, init_check_list, InitClock
// and INIT_REL_PIVOT, and mvba.hip's DevBufs, fail and MVBA_HIP.  Nothing here runs on the LM path.  
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
  if ((st & RS_ACTIVE) && i < ch_cnt[c] && rs_current(st, inl0, inl1)[ch_mask[c] + i]) {
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
    for (int e = 0; e < 144; ++e) sA[e * RS_HYP_BLOCK] = 0.0;
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
    double p[12];
    good = rs_lds_eig<12>(sA, sV, good, p);
    if (good) good = resect_denormalise(p, nm, P);
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
  const int mine = rs_score_block(nh, lane, live, [&](int hh) {
    double d2;
    return rr_inlier(s_P + 12 * hh, Xa, z, thr2, d2);
  });
  rs_score_add(mine, nh, lane, s_cnt, hyp_count + (size_t)kl * H + h0);
}

// Pcur[camera] = the 12 doubles (a matrix; R and t of a pose) of the camera's best hypothesis (best < 0: NaN), for the cnt
// cameras of a tile
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
    mask_step(in, d2, &rs_other(st, inl0, inl1)[ch_mask[c] + i], v);
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
  if (rs_current(st, inl0, inl1)[ch_mask[c] + i]) out[cm_obs[ch_start[c] + i]] = 1;
}

// What a fit sees of robust_cameras: the call, the current tile's cameras and chunks, and the buffers every fit uses (dP: the
// camera matrices that k_resect_mask scores, per listed camera).
struct CamTile {
  const CamWork &w;
  int H;
  unsigned long long seed;
  int c0, cnt, ch0, tch;
  dim3 gch, gc;  // one workgroup per chunk of the tile (at least one), one thread per camera
  const int *tcam, *tcnt;
  const long long *tstart, *tmask;
  double *dpart, *dS, *dP, *dhypP;
  int *dstate, *dhc;
  unsigned char *dinl0, *dinl1;
  // (a tile's sums: dS [cnt][nv], of the chunk partials at their global place in dpart)
  void combine(int nv) const { hipLaunchKernelGGL(k_resect_combine, dim3((cnt * nv + 255) / 256), dim3(256), 0, 0, cnt, nv, w.dlc_ch + c0, dpart, dS); }
};

// The robust fit of the listed cameras, tile by tile: hypotheses scored as camera matrices by k_resect_score, the best by
// rs_pick, its inlier mask, up to n_refit refits under the two-buffer mask and rs_accept, the scatter of the final mask, the
// per-camera outputs and the four laps.  A Fit (ResectFit below; PoseFit, mvba_pose_ransac.h) supplies
//   MIN_OBS, FIRST_MIN, NV (doubles per chunk partial), HYP_BYTES (device bytes per hypothesis of a camera of a tile),
//   setup: its own buffers;  hypotheses: whatever fills dhypP and dhc of a tile;  score_n: the counts k_resect_score goes by;
//   picked: after dP holds the best hypotheses;  fetch: after a mask, the model behind dP to the host (first: the kept one);
//   refit: one refit's model of the active cameras into dP, rs_stop for those that fail;  keep: refit model -> kept model;
//   output: the kept model of tile camera p to list position g, returns quality[g][1].
// The caller has checked its arguments and set the fit's own outputs to NaN.
template <class Fit>
int robust_cameras(Fit &fit, const double *X, int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int64_t n_obs,
                   int m, const uint8_t *point_ok, const double *K, const int32_t *cameras, int nl, double threshold, int H, uint64_t seed,
                   int n_refit, double *quality, int64_t *n_usable, int64_t *n_inliers, int32_t *best, uint8_t *inlier, int32_t *hyp_count,
                   int32_t *status, double *timings_ms, int32_t device) {
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = timings_ms[3] = 0.0;
  const double thr2 = threshold * threshold;
  // the defaults are those of a camera without usable observations: status 1
  RsTile::defaults((size_t)nl, H, status, best, hyp_count, n_usable, n_inliers, quality);
  if (inlier && n_obs) std::memset(inlier, 0, (size_t)n_obs);
  if (nl == 0) return MVBA_OK;

  InitClock clk;
  ResectList list;
  resect_build_list(X, n_points, pt_ptr, cam_idx, xy, m, point_ok, inlier != nullptr, list);
  const long long n_used = list.cam_ptr[m];
  CamWork w;
  int rc;
  if ((rc = w.build(list.cam_ptr.data(), cameras, nl, START_CHUNK, n_usable))) return rc;
  const int n_ch = w.n_ch;
  if (n_ch == 0) {
    if (timings_ms) timings_ms[0] = clk.lap();
    return MVBA_OK;
  }

  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  const int tile = tv_pair_tile(nl, Fit::HYP_BYTES * (size_t)H);
  DevBufs tmp;
  CamTile t{w, H, (unsigned long long)seed};
  int *dbest = nullptr;
  long long *dobs = nullptr;
  unsigned char *dout = nullptr;
  if ((rc = w.upload(tmp, list, X, n_points, K)) || (rc = tmp.alloc(&t.dpart, Fit::NV * (size_t)n_ch)) || (rc = tmp.alloc(&t.dS, Fit::NV * (size_t)tile)) ||
      (rc = tmp.alloc(&t.dP, 12 * (size_t)nl)) || (rc = tmp.alloc(&t.dstate, (size_t)nl)) || (rc = tmp.alloc(&dbest, (size_t)tile)) ||
      (rc = tmp.alloc(&t.dhc, (size_t)tile * H)) || (rc = tmp.alloc(&t.dhypP, 12 * (size_t)tile * H)) || (rc = tmp.alloc(&t.dinl0, (size_t)w.n_mask)) ||
      (rc = tmp.alloc(&t.dinl1, (size_t)w.n_mask)) || (rc = fit.setup(tmp, w, tile, H)))
    return rc;
  if (inlier && ((rc = tmp.alloc(&dout, (size_t)n_obs)) || (rc = tmp.alloc(&dobs, (size_t)n_used)))) return rc;
  if (inlier) {
    MVBA_HIP(hipMemcpy(dobs, list.cm_obs.data(), sizeof(long long) * n_used, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemset(dout, 0, (size_t)n_obs));
  }
  RsLaps laps;
  laps.upload = clk.lap();

  const dim3 b256(256), bch(START_CHUNK);
  const int hb = (H + RS_HYP_BLOCK - 1) / RS_HYP_BLOCK;
  std::vector<int> hc((size_t)tile * H), state((size_t)nl, 0);
  RsTile rt(tile);
  std::vector<double> S2(2 * (size_t)tile);
  for (int c0 = 0; c0 < nl; c0 += tile) {
    const int cnt = std::min(tile, nl - c0), ch0 = w.lc_ch[c0], tch = w.lc_ch[c0 + cnt] - ch0;
    t.c0 = c0; t.cnt = cnt; t.ch0 = ch0; t.tch = tch;
    t.gch = dim3((unsigned)std::max(tch, 1)); t.gc = dim3((cnt + 255) / 256);
    t.tcam = w.dch_cam + ch0; t.tcnt = w.dch_cnt + ch0; t.tstart = w.dch_start + ch0; t.tmask = w.dch_mask + ch0;
    int *tstate = state.data() + c0;
    auto put_state = [&]() -> int {
      MVBA_HIP(hipMemcpy(t.dstate + c0, tstate, sizeof(int) * cnt, hipMemcpyHostToDevice));
      return MVBA_OK;
    };
    // the inlier sets of dP under the cameras' states: counts and sums of d^2 into S2
    auto mask = [&]() -> int {
      int r = put_state();
      if (r) return r;
      if (tch > 0)
        hipLaunchKernelGGL(k_resect_mask, t.gch, bch, 0, 0, t.tcam, t.tstart, t.tmask, t.tcnt, w.dpt, w.dxy, w.dX, t.dstate, t.dP, thr2, t.dinl0, t.dinl1,
                           t.dpart + 2 * (size_t)ch0);
      t.combine(2);
      MVBA_HIP(hipGetLastError());
      MVBA_HIP(hipMemcpy(S2.data(), t.dS, sizeof(double) * 2 * cnt, hipMemcpyDeviceToHost));
      return MVBA_OK;
    };

    fit.hypotheses(t);
    if (tch > 0)
      hipLaunchKernelGGL(k_resect_score, dim3((unsigned)tch, hb), bch, 0, 0, c0, H, t.tcam, t.tstart, t.tcnt, fit.score_n(w), w.dpt, w.dxy, w.dX, t.dhypP,
                         thr2, t.dhc);
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(hc.data(), t.dhc, sizeof(int) * (size_t)cnt * H, hipMemcpyDeviceToHost));
    laps.score += clk.lap();

    rt.pick(cnt, tstate, hc.data(), H, w.lc_n.data() + c0, Fit::MIN_OBS);
    MVBA_HIP(hipMemcpy(dbest, rt.best.data(), sizeof(int) * cnt, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_resect_gather, dim3((cnt * 12 + 255) / 256), b256, 0, 0, cnt, H, dbest, t.dhypP, t.dP + 12 * (size_t)c0);
    fit.picked(t, dbest);
    if ((rc = mask()) || (rc = fit.fetch(t, true))) return rc;
    rt.first(S2.data(), [](int) { return 0; });  // (a hypothesis is a model as it is)
    laps.other += clk.lap();

    for (int r = 0; r < n_refit && rt.n_active > 0; ++r) {
      if ((rc = put_state()) || (rc = fit.refit(t, tstate, rt.n_active))) return rc;
      if (rt.n_active == 0) break;
      if ((rc = mask()) || (rc = fit.fetch(t, false))) return rc;
      rt.accept(r, S2.data(), Fit::FIRST_MIN, [&](int p) { fit.keep(p); });
    }
    laps.refit += clk.lap();

    if (inlier && tch > 0) {
      if ((rc = put_state())) return rc;
      hipLaunchKernelGGL(k_resect_scatter, t.gch, bch, 0, 0, t.tcam, t.tstart, t.tmask, t.tcnt, dobs, t.dstate, t.dinl0, t.dinl1, dout);
      MVBA_HIP(hipGetLastError());
    }
    rt.write((size_t)c0, status, best, hyp_count, n_inliers, quality, [&](int p) { return fit.output(p, (size_t)c0 + p); });
    laps.other += clk.lap();
  }
  if (inlier) MVBA_HIP(hipMemcpy(inlier, dout, (size_t)n_obs, hipMemcpyDeviceToHost));
  laps.other += clk.lap();
  laps.write(timings_ms);
  return MVBA_OK;
}

// The DLT as a fit: the normalisation over all usable observations before the hypotheses, a refit by mvba_resect's three
// passes under the mask and resect_solve_camera on the host.
struct ResectFit {
  static constexpr int MIN_OBS = RR_MIN_OBS, NV = 40;
  static constexpr size_t HYP_BYTES = RR_HYP_BYTES;
  // the first refit is kept if it has 6 inliers of its own (the minimal 6-point matrix is too ill-conditioned to hold the
  // full fit to its count), a later one while its set does not shrink
  static constexpr long long FIRST_MIN = RR_MIN_OBS;
  double *P;  // [n_cameras][12], out
  double *dnorm = nullptr, *dnorm2 = nullptr;
  int hyp_lds = 0;
  std::vector<double> S, norm, Pc, Pn, ratio, rt;

  int setup(DevBufs &tmp, const CamWork &w, int tile, int) {
    const size_t nl = w.cams.size();
    int rc;
    if ((rc = tmp.alloc(&dnorm, RS_NORM * nl)) || (rc = tmp.alloc(&dnorm2, RS_NORM * nl))) return rc;
    hyp_lds = (int)(sizeof(double) * 2 * 144 * RS_HYP_BLOCK);
    MVBA_HIP(hipFuncSetAttribute((const void *)k_resect_hyp, hipFuncAttributeMaxDynamicSharedMemorySize, hyp_lds));
    S.resize(40 * (size_t)tile); norm.resize(RS_NORM * (size_t)tile); Pc.resize(12 * (size_t)tile); Pn.resize(12 * (size_t)tile);
    ratio.resize((size_t)tile); rt.resize((size_t)tile);
    return MVBA_OK;
  }
  const int *score_n(const CamWork &w) const { return w.dlc_n; }
  // normalisation over all usable observations (mvba_resect's passes 0 and 1), hypotheses
  void hypotheses(const CamTile &t) {
    const CamWork &w = t.w;
    const dim3 b256(256), bch(START_CHUNK);
    if (t.tch > 0) {
      hipLaunchKernelGGL(k_resect_chunk<0>, t.gch, bch, 0, 0, t.tcam, t.tstart, t.tcnt, w.dpt, w.dxy, w.dX, (const double *)nullptr, t.dpart + 6 * (size_t)t.ch0);
      t.combine(6);
      hipLaunchKernelGGL(k_resect_norm, t.gc, b256, 0, 0, t.cnt, 0, t.dS, dnorm + RS_NORM * (size_t)t.c0);
      hipLaunchKernelGGL(k_resect_chunk<1>, t.gch, bch, 0, 0, t.tcam, t.tstart, t.tcnt, w.dpt, w.dxy, w.dX, dnorm, t.dpart + 2 * (size_t)t.ch0);
      t.combine(2);
      hipLaunchKernelGGL(k_resect_norm, t.gc, b256, 0, 0, t.cnt, 1, t.dS, dnorm + RS_NORM * (size_t)t.c0);
    }
    hipLaunchKernelGGL(k_resect_hyp, dim3((t.H + RS_HYP_BLOCK - 1) / RS_HYP_BLOCK, t.cnt), dim3(RS_HYP_BLOCK), hyp_lds, 0, t.c0, t.H, t.seed, w.dcams,
                       w.dlc_start, w.dlc_n, w.dpt, w.dxy, w.dX, dnorm, t.dhypP, t.dhc);
  }
  void picked(const CamTile &, const int *) {}
  int fetch(const CamTile &t, bool first) {
    if (!first) return MVBA_OK;  // (a refit's matrices came from the host)
    MVBA_HIP(hipMemcpy(Pc.data(), t.dP + 12 * (size_t)t.c0, sizeof(double) * 12 * t.cnt, hipMemcpyDeviceToHost));
    std::fill(ratio.begin(), ratio.end(), 0.0);  // (no refit kept yet)
    return MVBA_OK;
  }
  // mvba_resect's fit on the current inliers alone
  int refit(const CamTile &t, int *tstate, int &n_active) {
    const CamWork &w = t.w;
    const dim3 b256(256), bch(START_CHUNK);
    double *tn = dnorm2 + RS_NORM * (size_t)t.c0;
    hipLaunchKernelGGL(k_resect_fit<0>, t.gch, bch, 0, 0, t.tcam, t.tstart, t.tmask, t.tcnt, w.dpt, w.dxy, w.dX, t.dstate, t.dinl0, t.dinl1,
                       (const double *)nullptr, t.dpart + 6 * (size_t)t.ch0);
    t.combine(6);
    hipLaunchKernelGGL(k_resect_norm, t.gc, b256, 0, 0, t.cnt, 0, t.dS, tn);
    hipLaunchKernelGGL(k_resect_fit<1>, t.gch, bch, 0, 0, t.tcam, t.tstart, t.tmask, t.tcnt, w.dpt, w.dxy, w.dX, t.dstate, t.dinl0, t.dinl1, dnorm2,
                       t.dpart + 2 * (size_t)t.ch0);
    t.combine(2);
    hipLaunchKernelGGL(k_resect_norm, t.gc, b256, 0, 0, t.cnt, 1, t.dS, tn);
    hipLaunchKernelGGL(k_resect_fit<2>, t.gch, bch, 0, 0, t.tcam, t.tstart, t.tmask, t.tcnt, w.dpt, w.dxy, w.dX, t.dstate, t.dinl0, t.dinl1, dnorm2,
                       t.dpart + 40 * (size_t)t.ch0);
    t.combine(40);
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(S.data(), t.dS, sizeof(double) * 40 * t.cnt, hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(norm.data(), tn, sizeof(double) * RS_NORM * t.cnt, hipMemcpyDeviceToHost));
    std::fill(rt.begin(), rt.end(), NAN);
    for (int p = 0; p < t.cnt; ++p) {
      for (int j = 0; j < 12; ++j) Pn[12 * (size_t)p + j] = NAN;
      if (!(tstate[p] & RS_ACTIVE)) continue;
      if (resect_solve_camera(S.data() + 40 * (size_t)p, norm.data() + RS_NORM * (size_t)p, Pn.data() + 12 * (size_t)p, &rt[p])) rs_stop(tstate[p], n_active);
    }
    if (n_active > 0) MVBA_HIP(hipMemcpy(t.dP + 12 * (size_t)t.c0, Pn.data(), sizeof(double) * 12 * t.cnt, hipMemcpyHostToDevice));
    return MVBA_OK;
  }
  void keep(int p) {
    ratio[p] = rt[p];
    for (int j = 0; j < 12; ++j) Pc[12 * (size_t)p + j] = Pn[12 * (size_t)p + j];
  }
  double output(int p, size_t g) const {
    for (int j = 0; j < 12; ++j) P[12 * g + j] = Pc[12 * (size_t)p + j];
    return ratio[p];
  }
};

}  // namespace

extern "C" {

int mvba_resect_sample(uint64_t seed, int32_t k, int32_t h, int64_t n, int64_t *idx6) {
  return sample_entry<RR_MIN_OBS>(seed, "kh", k, k, h, n, idx6, "idx6", 5);
}

int mvba_resect_robust(const double *X, int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int64_t n_obs,
                       int32_t n_images, const uint8_t *point_ok, const int32_t *cameras, int32_t n_cameras, double threshold,
                       int32_t n_hypotheses, uint64_t seed, int32_t n_refit, double *P, double *quality, int64_t *n_usable,
                       int64_t *n_inliers, int32_t *best, uint8_t *inlier, int32_t *hyp_count, int32_t *status, double *timings_ms,
                       int32_t device) {
  if (n_cameras < 0) return fail(MVBA_ERR_BADARG, "n_cameras = " + std::to_string(n_cameras) + " must be >= 0");
  if (!X || !xy || (n_cameras > 0 && !P))
    return fail(MVBA_ERR_BADARG, std::string("null argument: ") + (!X ? "X" : (!xy ? "xy" : "P")) + " (argument " + std::to_string(!X ? 1 : (!xy ? 5 : 15)) + ")");
  int rc;
  if ((rc = rs_check_search(threshold, n_hypotheses)) || (rc = rs_check_refit(n_refit)) ||
      (rc = init_check_list(n_points, n_images, pt_ptr, cam_idx, n_obs)) || (rc = check_camera_list(cameras, n_cameras, n_images)))
    return rc;
  std::fill(P, P + 12 * (size_t)n_cameras, NAN);
  ResectFit fit{P};
  return robust_cameras(fit, X, n_points, pt_ptr, cam_idx, xy, n_obs, n_images, point_ok, nullptr, cameras, n_cameras, threshold, n_hypotheses, seed,
                        n_refit, quality, n_usable, n_inliers, best, inlier, hyp_count, status, timings_ms, device);
}

}  // extern "C"
